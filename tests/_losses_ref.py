"""numpy restatements of the three loss formulas and of the pair distance, shared by test_losses_host.py (which checks them
against the reference fixtures) and test_gpu_losses.py."""
import numpy as np


def sqdist(xT_rows, xS_rows):
    """d2 per row pair in the arrays' dtype: channels ascending, every operation rounded on its own (numpy never contracts)."""
    t = xT_rows[..., 0] - xS_rows[..., 0]
    acc = t * t
    for c in range(1, xT_rows.shape[-1]):
        t = xT_rows[..., c] - xS_rows[..., c]
        acc = acc + t * t
    return acc


def dense_sqdist(xT, xS, block=256):
    """(N_T, N_S) matrix of sqdist, built in row blocks"""
    out = np.empty((xT.shape[0], xS.shape[0]), dtype=xT.dtype)
    for a in range(0, xT.shape[0], block):
        out[a:a + block] = sqdist(xT[a:a + block, None, :], xS[None, :, :])
    return out


def twin_loss(xS, xT, p, n, yN, mu):
    """float64 loss and gradients (gS, gT) of the twin loss"""
    rest = (np.float32(1) - yN.astype(np.float32)).astype(np.float64)          # the reference subtracts in float32
    xS, xT, yN = xS.astype(np.float64), xT.astype(np.float64), yN.astype(np.float64)
    P, M = p.shape[0], n.shape[0]
    tp = xT[p[:, 0]] - xS[p[:, 1]]
    tn = xT[n[:, 0]] - xS[n[:, 1]]
    dp, dn = (tp * tp).sum(1), (tn * tn).sum(1)
    loss_p = dp.sum() / P
    loss_n = ((yN * dn).sum() + (rest * np.maximum(mu - dn, 0)).sum()) / M
    cn = 2.0 * (yN - rest * (mu - dn > 0)) / M
    gT, gS = np.zeros_like(xT), np.zeros_like(xS)
    np.add.at(gT, p[:, 0], 2.0 / P * tp)
    np.add.at(gS, p[:, 1], -2.0 / P * tp)
    np.add.at(gT, n[:, 0], cn[:, None] * tn)
    np.add.at(gS, n[:, 1], -cn[:, None] * tn)
    return loss_p, loss_n, gS, gT


def label_smoothing(pred, target, classes, smoothing, weight=None):
    """float64 loss and gradient of the label-smoothing loss"""
    x = pred.astype(np.float64)
    N, K = x.shape
    w = np.ones(K) if weight is None else weight.astype(np.float64)
    t = np.full((N, K), smoothing / (classes - 1))
    t[np.arange(N), target] = 1.0 - smoothing
    z = x - x.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1, keepdims=True))
    logp = z - lse
    loss = (-(t * w) * logp).sum(1).mean()
    grad = (np.exp(logp) * (t * w).sum(1, keepdims=True) - t * w) / N
    return loss, grad


def parse_variant(v):
    """'s1_w_c43_f64' -> (smoothing, weighted, classes, numpy dtype)"""
    s, w, c, tag = v.split('_')
    return int(s[1:]) / 10.0, w == 'w', int(c[1:]), np.float32 if tag == 'f32' else np.float64
