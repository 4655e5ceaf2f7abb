"""fp64 restatement of the FEARec contract (bsarec_amd/fearec.py, include/bsarec_hip.h): the band table, the band-limited
autocorrelation attention in its frequency-domain form (explicit DFT sums in numpy), its derivative with the delays held fixed,
and a small fp64 torch twin of the whole model with dropout 0.  Shared by tests/test_fearec_cpu.py and the GPU tests."""
import math

import numpy as np
import torch


# ---- the band table and k --------------------------------------------------------------------------------------------------
def bands(L, N, gamma):
    F = L // 2 + 1
    if N > 1 and gamma > 1.0 / N:
        w, s = gamma, (F * (1 - gamma)) // (N - 1)
    elif N > 1:
        w, s = 1.0 / N, F / N
    else:
        w, s = max(gamma, 1.0 / N), 0
    out = []
    for i in range(N):
        lo, hi = int(F * (1 - w) - i * s), int(F - i * s)
        if not 0 <= lo < hi <= F:
            raise ValueError(f"band [{lo}, {hi}) of layer {i}")
        out.append((lo, hi))
    return out


def topk(L, factor=1.0):
    return max(1, min(int(factor * math.log(L)), L, 32))


# ---- the layer in numpy ----------------------------------------------------------------------------------------------------
def _phase(L, lo, hi):
    """e^{-2 pi i f t / L} [nb, L] from exactly reduced arguments, and w_f [nb]."""
    f = np.arange(lo, hi)[:, None]
    t = np.arange(L)[None, :]
    ang = ((f * t) % L).astype(np.float64) * (2.0 * np.pi / L)
    w = np.where((f[:, 0] == 0) | (2 * f[:, 0] == L), 1.0, 2.0)
    return np.exp(-1j * ang), w


def spectra(X, lo, hi):
    """Xf[b, f, c] = sum_t X[b, t, c] e^{-2 pi i f t / L}, f in the band."""
    E, _ = _phase(X.shape[1], lo, hi)
    return np.einsum("ft,btc->bfc", E, X.astype(np.float64))


def mean_corr(Q, K, lo, hi):
    """m [B, L] (contract, steps 1-3)."""
    B, L, D = Q.shape
    E, w = _phase(L, lo, hi)
    S = (spectra(Q, lo, hi) * np.conj(spectra(K, lo, hi))).sum(-1)             # [B, nb]
    return np.real(np.einsum("bf,ft->bt", S * w, np.conj(E))) / (D * L)      # e^{+i theta f tau}


def select(values, k):
    """The k indices with the largest values along the last axis, ties to the lower index."""
    return np.argsort(-values, axis=-1, kind="stable")[..., :k]


def ambiguous(values, k, margin, exact_ties=False):
    """Per row of ``values`` [..., L]: is the gap between the k-th and the (k+1)-th largest below margin * max|values|?
    ``exact_ties``: a gap of exactly 0 is not ambiguous -- the rule (the lower index) decides it.  Only for bands whose m repeats
    bit for bit by construction (DC alone, the Nyquist bin alone)."""
    v = -np.sort(-values, axis=-1)
    if k >= v.shape[-1]:
        return np.zeros(v.shape[:-1], dtype=bool)
    gap = v[..., k - 1] - v[..., k]
    amb = gap < margin * np.abs(values).max()
    return amb & (gap != 0) if exact_ties else amb


def _softmax(x):
    e = np.exp(x - x.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def _idx_rows(idx, B):
    return np.broadcast_to(idx, (B, idx.shape[-1])) if idx.ndim == 1 else idx


def forward(Q, K, V, lo, hi, k, train, idx=None):
    """(out [B, L, D], m [B, L], idx ([k] in training mode, [B, k] otherwise), p [B, k]); ``idx`` given: held fixed."""
    B, L, D = Q.shape
    m = mean_corr(Q, K, lo, hi)
    if idx is None:
        idx = select(m.mean(0), k) if train else select(m, k)
    rows = _idx_rows(idx, B)
    p = _softmax(np.take_along_axis(m, rows, axis=1))
    V = V.astype(np.float64)
    out = np.zeros((B, L, D))
    t = np.arange(L)
    for b in range(B):
        for i in range(rows.shape[1]):
            out[b] += p[b, i] * V[b, (t + rows[b, i]) % L]
    return out, m, idx, p


def backward(Q, K, V, dOut, lo, hi, idx, absolute=False):
    """(dQ, dK, dV) of sum(out * dOut) with idx fixed.  ``absolute``: with |dm| in place of dm -- the size dQ and dK have when the
    delays' terms do not cancel, a scale for the cases in which they cancel identically."""
    B, L, D = Q.shape
    k = idx.shape[-1]
    m = mean_corr(Q, K, lo, hi)
    rows = _idx_rows(idx, B)
    p = _softmax(np.take_along_axis(m, rows, axis=1))
    V, dOut = V.astype(np.float64), dOut.astype(np.float64)
    t = np.arange(L)
    dV, dp = np.zeros((B, L, D)), np.zeros((B, k))
    for b in range(B):
        for i in range(k):
            src = (t + rows[b, i]) % L
            dp[b, i] = (dOut[b] * V[b, src]).sum()
            np.add.at(dV[b], src, p[b, i] * dOut[b])
    dsel = p * (dp - (p * dp).sum(-1, keepdims=True))
    if absolute:
        dsel = np.abs(dsel)
    dm = np.zeros((B, L))
    for b in range(B):
        np.add.at(dm[b], rows[b], dsel[b])
    E, w = _phase(L, lo, hi)
    g = np.einsum("bt,ft->bf", dm, E) * w / (D * L)         # dRe S + i dIm S = w_f / (D L) sum_tau dm[tau] e^{-i theta f tau}
    Qf, Kf = spectra(Q, lo, hi), spectra(K, lo, hi)
    dQ = np.real(np.einsum("bfc,ft->btc", g[:, :, None] * Kf, np.conj(E)))
    dK = np.real(np.einsum("bfc,ft->btc", np.conj(g)[:, :, None] * Qf, np.conj(E)))
    return dQ, dK, dV


def random_case(shape, seed):
    """Q, K, V ~ N(0, 1), rounded to fp32; shape = (B, L, D)."""
    rng = np.random.default_rng(seed)
    return tuple(rng.standard_normal(shape).astype(np.float32) for _ in range(3))


def rel_l2(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- the layer in torch (any dtype; differentiable with the delays fixed, as the contract has it) ------------------------------
def torch_attention(q, k, v, lo, hi, kk, train, margin=None, idx=None):
    """The literal restatement: rfft, band mask, irfft(n = L), channel mean, top-k, softmax, rolls.  ``margin``: assert that the
    choice of the delays is not ambiguous (g in training mode, every row in evaluation mode).  ``idx`` [B, k]: delays given, not
    chosen."""
    B, L, D = q.shape
    res = torch.fft.rfft(q, dim=1) * torch.conj(torch.fft.rfft(k, dim=1))
    box = torch.zeros_like(res)
    box[:, lo:hi] = res[:, lo:hi]
    m = torch.fft.irfft(box, n=L, dim=1).mean(-1)                              # [B, L]
    with torch.no_grad():
        if idx is not None:
            idx = torch.as_tensor(np.array(idx), dtype=torch.int64, device=q.device)
        elif train:
            g = m.mean(0)
            if margin is not None:
                assert not ambiguous(g.double().cpu().numpy(), kk, margin), "ambiguous delays: pick another seed"
            idx = torch.sort(-g, stable=True).indices[:kk][None].expand(B, kk)
        else:
            if margin is not None:
                assert not ambiguous(m.double().cpu().numpy(), kk, margin).any(), "ambiguous delays: pick another seed"
            idx = torch.sort(-m, dim=1, stable=True).indices[:, :kk]
    p = torch.softmax(m.gather(1, idx), dim=1)
    t = torch.arange(L, device=q.device)
    out = torch.zeros_like(v)
    for i in range(kk):
        src = (t[None, :] + idx[:, i:i + 1]) % L                               # [B, L]
        out = out + p[:, i, None, None] * v.gather(1, src[:, :, None].expand(B, L, D))
    return out, m, idx


# ---- the whole model in fp64 torch, dropout 0 --------------------------------------------------------------------------------
def _ln(x, w, b, eps=1e-12):
    xc = x - x.mean(-1, keepdim=True)
    return w * (xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + eps)) + b


def _info_nce(zi, zj, tau, sim):
    B = zi.shape[0]
    z = torch.cat((zi, zj), 0)
    if sim == "cos":
        z = z / z.norm(dim=1, keepdim=True).clamp_min(1e-8)
    s = z @ z.T / tau
    s = s.masked_fill(torch.eye(2 * B, dtype=torch.bool), -math.inf)
    pos = torch.cat((torch.arange(B) + B, torch.arange(B)))
    return torch.nn.functional.cross_entropy(s, pos)


class Twin:
    """fp64 CPU twin of FEARecModel with dropout 0: ``params`` are leaf tensors named like the state_dict."""

    def __init__(self, state_dict, args, margin=1e-4):
        self.p = {k: v.detach().double().cpu().clone().requires_grad_(True) for k, v in state_dict.items()}
        self.a, self.margin = args, margin
        self.L, self.N = args.max_seq_length, args.num_hidden_layers
        self.bands = bands(self.L, self.N, getattr(args, "global_ratio", 0.6))
        self.k = topk(self.L, getattr(args, "fea_topk_factor", 1.0))
        self.r = getattr(args, "spatial_ratio", 0.1)

    def encode(self, ids, train):
        P, L = self.p, self.L
        ids = ids.cpu().long()
        B = ids.shape[0]
        d, h = self.a.hidden_size, self.a.num_attention_heads
        x = _ln(P["item_embeddings.weight"][ids] + P["position_embeddings.weight"][None, :L], P["LayerNorm.weight"], P["LayerNorm.bias"])
        ok = (ids > 0)[:, None, None, :] & torch.tril(torch.ones(L, L, dtype=torch.bool))[None, None]
        mask = (1.0 - ok.double()) * -10000.0
        lin = lambda t, n: t @ P[n + ".weight"].T + P[n + ".bias"]
        for i, (lo, hi) in enumerate(self.bands):
            pre = f"item_encoder.blocks.{i}."
            q, k, v = (lin(x, pre + "layer." + n) for n in ("query", "key", "value"))
            ctx = torch_attention(q, k, v, lo, hi, self.k, train, self.margin)[0]
            if self.r > 0:
                qh, kh, vh = (t.view(B, L, h, d // h).transpose(1, 2) for t in (q, k, v))
                a = torch.softmax(qh @ kh.transpose(-1, -2) / math.sqrt(d // h) + mask, -1)
                ctx = (1 - self.r) * ctx + self.r * (a @ vh).transpose(1, 2).reshape(B, L, d)
            hdn = _ln(lin(ctx, pre + "layer.dense") + x, P[pre + "layer.LayerNorm.weight"], P[pre + "layer.LayerNorm.bias"])
            u = lin(hdn, pre + "feed_forward.dense_1")
            u = u * 0.5 * (1.0 + torch.erf(u / math.sqrt(2.0)))
            x = _ln(lin(u, pre + "feed_forward.dense_2") + hdn, P[pre + "feed_forward.LayerNorm.weight"],
                    P[pre + "feed_forward.LayerNorm.bias"])
        return x

    @staticmethod
    def spectral_distance(a, b):
        return torch.abs(torch.fft.rfft(a, dim=1, norm="ortho") - torch.fft.rfft(b, dim=1, norm="ortho")).mean()

    def loss(self, ids, answers, same_target):
        a = self.a
        ssl, tau, sim = getattr(a, "ssl", "us_x"), getattr(a, "tau", 1.0), getattr(a, "sim", "dot")
        lmd, lmd_sem = getattr(a, "lmd", 0.1), getattr(a, "lmd_sem", 0.1)
        seq = self.encode(ids, True)
        loss = torch.nn.functional.cross_entropy(seq[:, -1] @ self.p["item_embeddings.weight"].T, answers.cpu().long())
        if ssl in ("us", "un"):
            aug = self.encode(ids, True)
            loss = loss + lmd * _info_nce(seq[:, -1], aug[:, -1], tau, sim)
        if ssl in ("us", "su"):
            sem = self.encode(same_target, True)
            loss = loss + lmd_sem * _info_nce(seq[:, -1], sem[:, -1], tau, sim)
        if ssl == "us_x":
            aug, sem = self.encode(ids, True), self.encode(same_target, True)
            loss = loss + lmd_sem * _info_nce(aug[:, -1], sem[:, -1], tau, sim)
            if getattr(a, "fredom", True):
                ft = getattr(a, "fredom_type", "us_x")
                if ft in ("un", "us_x"):
                    loss = loss + 0.1 * self.spectral_distance(seq, aug)
                if ft in ("su", "us_x"):
                    loss = loss + 0.1 * self.spectral_distance(seq, sem)
        return loss
