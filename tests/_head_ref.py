"""numpy float64 restatement of the fused classification head (fieldconv_amd.head): the loss of `cross_entropy(h W^T + b, target)`
with this package's label-smoothing convention, its three gradients, and the prediction order.  The contract the GPU tests
compare the kernels with; tests/test_head_host.py pins it to torch on the CPU."""
import numpy as np


def logits(h, W, b=None):
    z = h.astype(np.float64) @ W.astype(np.float64).T
    return z if b is None else z + b.astype(np.float64)


def row_weights(target, K, smoothing, ignore_index=-100):
    """(q (N,K), counted (N,) bool, bad (N,) bool): the true class weighs 1 - smoothing, every other class smoothing / (K - 1);
    rows whose target is ignore_index have q = 0 and do not count; any other target outside [0,K) is `bad`."""
    target = np.asarray(target)
    N = target.shape[0]
    counted = target != ignore_index
    bad = counted & ((target < 0) | (target >= K))
    good = counted & ~bad
    q = np.zeros((N, K))
    if smoothing > 0:
        q[good] = smoothing / (K - 1)
    q[np.nonzero(good)[0], target[good]] = 1.0 - smoothing
    return q, counted, bad


def logsumexp(z):
    m = z.max(1, keepdims=True)
    return (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]


def loss_rows(z, target, smoothing=0.0, ignore_index=-100):
    """(N,) per-row losses of float64 logits: lse - sum_k q z; 0 for an ignored row, NaN for a bad one"""
    q, counted, bad = row_weights(target, z.shape[1], smoothing, ignore_index)
    rows = np.where(counted, logsumexp(z) - (q * z).sum(1), 0.0)
    rows[bad] = np.nan
    return rows


def reduce_rows(rows, target, reduction, ignore_index=-100):
    """'none', or the rows added in index order in float64 ('sum'), divided by the number of rows that count ('mean')"""
    if reduction == 'none':
        return rows
    s = 0.0
    for v in np.asarray(rows, dtype=np.float64):
        s += v
    if reduction == 'sum':
        return s
    n = int((np.asarray(target) != ignore_index).sum())
    return s / n if n else np.nan


def head(h, W, b, target, reduction='mean', smoothing=0.0, ignore_index=-100, upstream=None):
    """(loss, g_h, g_W, g_b) in float64.  upstream: the cotangent of the loss ((N,) for 'none', a number otherwise; default
    ones).  A bad row makes its row of G -- and so its row of g_h and all of g_W, g_b -- NaN, like its loss."""
    z = logits(h, W, b)
    N, K = z.shape
    q, counted, bad = row_weights(target, K, smoothing, ignore_index)
    rows = loss_rows(z, target, smoothing, ignore_index)
    loss = reduce_rows(rows, target, reduction, ignore_index)
    if reduction == 'none':
        g = np.ones(N) if upstream is None else np.asarray(upstream, dtype=np.float64)
    else:
        g = np.full(N, 1.0 if upstream is None else float(upstream))
        if reduction == 'mean':
            g = g / max(int(counted.sum()), 1)
    p = np.exp(z - logsumexp(z)[:, None])
    G = np.where(counted[:, None], g[:, None] * (p - q), 0.0)
    G[bad] = np.nan
    return loss, G @ W.astype(np.float64), G.T @ h.astype(np.float64), G.sum(0)


def topk(z, k):
    """(idx (N,k) int64, zk (N,k) of z's dtype): per row the classes ordered by (logit descending, class ascending), a NaN
    after every number (NaNs among themselves by class); slots beyond K hold -1 / -inf."""
    N, K = z.shape
    idx = np.full((N, k), -1, dtype=np.int64)
    zk = np.full((N, k), -np.inf, dtype=z.dtype)
    for n in range(N):
        order = sorted(range(K), key=lambda c: (1, 0.0, c) if np.isnan(z[n, c]) else (0, -float(z[n, c]), c))[:k]
        idx[n, :len(order)] = order
        zk[n, :len(order)] = z[n, order]
    return idx, zk


def accuracy(idx, target, ignore_index=-100):
    """(k,) float64: entry j the share of the counted rows whose target is among idx[n, :j + 1], by a direct count"""
    target = np.asarray(target)
    rows = [n for n in range(len(target)) if target[n] != ignore_index and target[n] >= 0]
    hits = np.zeros(idx.shape[1])
    for n in rows:
        for j in range(idx.shape[1]):
            if target[n] in idx[n, :j + 1]:
                hits[j] += 1
    return hits / np.float64(len(rows))
