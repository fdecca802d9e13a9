"""numpy restatement of descriptor matching (fieldconv_amd.matching, csrc/fc_match.hip), shared by test_matching_host.py (which
checks it against a brute-force double loop) and test_gpu_matching.py.  The distance is _losses_ref.sqdist, bit for bit; the
selection is np.lexsort on (b, d2) per row with NaN distances dropped, per segment, with one row of xS excluded per row of xT."""
import numpy as np

import _losses_ref as ref


def _segments(n_T, n_S, ptr_S, ptr_T):
    if ptr_T is None:
        return [(0, n_T, 0, n_S)]
    return [(int(ptr_T[m]), int(ptr_T[m + 1]), int(ptr_S[m]), int(ptr_S[m + 1])) for m in range(len(ptr_T) - 1)]


def topk(xS, xT, k, ptr_S=None, ptr_T=None, exclude=None, rows=None):
    """(idx (R,k) int64, d2 (R,k) in the features' dtype) for the xT rows `rows` (all of them when None), in that order:
    the k rows b of xS (of a's segment, without exclude[a]) with the smallest (d2, b); empty slots hold -1 / +inf."""
    n_T, n_S = xT.shape[0], xS.shape[0]
    rows = np.arange(n_T) if rows is None else np.asarray(rows)
    idx = np.full((rows.size, k), -1, dtype=np.int64)
    d2 = np.full((rows.size, k), np.inf, dtype=xT.dtype)
    for t0, t1, s0, s1 in _segments(n_T, n_S, ptr_S, ptr_T):
        mine = np.nonzero((rows >= t0) & (rows < t1))[0]
        if not mine.size or s1 <= s0:
            continue
        with np.errstate(invalid='ignore', over='ignore'):
            D = ref.dense_sqdist(xT[rows[mine]], xS[s0:s1])
        b = np.arange(s0, s1)
        for r, drow in zip(mine, D):
            keep = ~np.isnan(drow)
            if exclude is not None:
                keep &= b != exclude[rows[r]]
            cb, cd = b[keep], drow[keep]
            order = np.lexsort((cb, cd))[:k]
            idx[r, :order.size] = cb[order]
            d2[r, :order.size] = cd[order]
    return idx, d2


def mutual(xS, xT, ptr_S=None, ptr_T=None):
    """(M,2) rows [a, b], a ascending: b is the nearest row of a and a the nearest row of b"""
    to_S = topk(xS, xT, 1, ptr_S, ptr_T)[0][:, 0]
    to_T = topk(xT, xS, 1, ptr_T, ptr_S)[0][:, 0]
    out = [(a, b) for a, b in enumerate(to_S) if b >= 0 and to_T[b] == a]
    return np.array(out, dtype=np.int64).reshape(-1, 2)


def accuracy(idx, pos):
    """(k,) float64: the share of the distinct rows pos[:,0] with one of their true rows among idx[a, :j + 1]"""
    rows = np.unique(pos[:, 0])
    out = np.zeros(idx.shape[1])
    for j in range(idx.shape[1]):
        out[j] = sum(any(b in idx[a, :j + 1] for b in pos[pos[:, 0] == a, 1]) for a in rows) / rows.size
    return out


def hard_negatives(xS, xT, pos, per_row):
    """(R * per_row, 2) rows [a, b]: for each distinct row a of pos (ascending), its per_row nearest rows that are not its positive"""
    exclude = np.full(xT.shape[0], -1, dtype=np.int64)
    exclude[pos[:, 0]] = pos[:, 1]
    rows = np.unique(pos[:, 0])
    idx, _ = topk(xS, xT, per_row, exclude=exclude, rows=rows)
    out = [(a, b) for a, near in zip(rows, idx) for b in near if b >= 0]
    return np.array(out, dtype=np.int64).reshape(-1, 2)
