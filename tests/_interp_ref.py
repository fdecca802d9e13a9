"""numpy restatement of fieldconv_amd.transfer.interpolation_plan (csrc/fc_interp.hip): the selection of the k nearest candidates
and their inverse-distance weights with float32 operations in the kernel's order (or float64, the yardstick of the method), the
candidate relation from the bounded float32 fields of _logmap_ref / _geodesic_sampling_ref, and the rows of the plan.  Built on
_transfer_ref (graphs, cells), imported unchanged.  Uses nothing from the package."""
import numpy as np

import _logmap_ref as lref
import _transfer_ref as tref

F32 = np.float32


# ------------------------------------------------------------------ selection and weights
def knn_weights(rowptr, cand, dist, k, power, real=F32):
    """(sel (n_f,k) int32, weight (n_f,k) real): per row the m = min(k, length) smallest slots by (dist, cand, slot) in that
    order, -1 beyond; weights 1, 0, ..., 0 when the nearest distance is 0, else u_i / s with q_i = d_i or d_i * d_i,
    u_i = 1 / max(q_i, 1e-30), s = ((u_0 + u_1) + u_2) + ..., every operation rounded to `real`; 0 beyond m"""
    assert 1 <= k <= 16 and power in (1, 2)
    n_f = len(rowptr) - 1
    sel = np.full((n_f, k), -1, dtype=np.int32)
    weight = np.zeros((n_f, k), dtype=real)
    d_all = np.asarray(dist).astype(real)
    for f in range(n_f):
        slots = np.arange(rowptr[f], rowptr[f + 1])
        if not len(slots):
            continue
        order = np.lexsort((slots, cand[slots], d_all[slots]))          # the last key is the first to decide
        pick = slots[order[:k]]
        m = len(pick)
        d = d_all[pick]
        sel[f, :m] = pick
        if d[0] == 0:
            weight[f, 0] = 1
            continue
        q = d * d if power == 2 else d
        u = real(1) / np.maximum(q, real(1e-30))
        s = u[0]
        for i in range(1, m):
            s = s + u[i]
        assert u.dtype == real and type(s) == real
        weight[f, :m] = u / s
    return sel, weight


def plan_rows(rowptr, cand, xp, sel, weight):
    """(rows (E,2) int64 [f, c], weight (E,), phase (E,)) in the plan's slot order: by receiver, then rank"""
    taken = sel >= 0
    slot = sel[taken]
    recv = np.nonzero(taken)[0]
    return np.stack((recv, cand[slot].astype(np.int64)), 1), weight[taken], xp[slot]


# ------------------------------------------------------------------ radius and candidates
def default_radius(pos, face, sample_idx, coarse, diagonals=False):
    """fl32(2 far) one float32 step upward, far the largest finite cell distance; None when far == 0"""
    cell, dist = tref.sample_cells(pos, face, sample_idx, coarse, diagonals)
    inside = (cell >= 0) & np.isfinite(dist)
    far = dist[inside].max() if inside.any() else F32(0)
    return float(np.nextafter(F32(2) * F32(far), F32(np.inf))) if far > 0 else None


def candidates(pos, face, sample_idx, coarse, radius, diagonals=False):
    """(rowptr (S_f+1,) int32, cand (E,) int32, field (E,) float32): the CSR by receiver f of every coarse position c whose
    field from vertex sample_idx[coarse[c]], bounded by radius, is < fl32(radius) (strict) at vertex sample_idx[f]; c ascending
    in a row"""
    graph = tref.graph_of(pos, face, diagonals)
    S_f = len(sample_idx)
    pairs = []
    for c, a in enumerate(coarse):
        d = lref.bounded_field(*graph, sample_idx[a], radius)[sample_idx]
        pairs += [(f, c, d[f]) for f in np.nonzero(d < F32(radius))[0]]
    pairs.sort(key=lambda t: (t[0], t[1]))
    f = np.array([p[0] for p in pairs], dtype=np.int64)
    rowptr = np.searchsorted(f, np.arange(S_f + 1)).astype(np.int32)
    return rowptr, np.array([p[1] for p in pairs], dtype=np.int32), np.array([p[2] for p in pairs], dtype=F32)


# ------------------------------------------------------------------ crafted rows for the kernel
def crafted_csr(k, seed=0, n_f=300):
    """(rowptr, cand, dist) of n_f rows: empty rows, rows of length 1, k - 1, k, k + 1, one row of 200, duplicate distances with
    different cand, identical (dist, cand) pairs, zero distances at rank 0 and at two slots, and a distance of 1e-25"""
    rng = np.random.default_rng(seed + 100 * k)
    rows = []

    def row(n):
        return list(zip(rng.integers(0, 50, n).tolist(), (rng.random(n) * 2 + 0.01).astype(F32).tolist()))
    for f in range(n_f):
        rows.append(row(int(rng.integers(2, 41))))
    for f, n in ((0, 0), (7, 0), (n_f - 1, 0), (1, 1), (2, max(k - 1, 0)), (3, k), (4, k + 1), (5, 200)):
        rows[f] = row(n)
    rows[8] = [(9, 0.5), (4, 0.5), (6, 0.25), (2, 0.5), (4, 0.5), (7, 0.75)]          # equal distances, other cand; (0.5, 4) twice
    rows[9] = [(3, 0.5), (3, 0.5), (3, 0.5), (1, 0.5)]
    rows[10] = [(5, 0.3), (8, 0.0), (2, 0.7), (6, 0.9)]                                 # a zero at rank 0
    rows[11] = [(5, 0.3), (8, 0.0), (2, 0.0), (6, 0.9), (1, 0.1)]                       # zeros at two slots
    rows[12] = [(5, 1e-25), (8, 0.4), (2, 0.2)]                                         # under the clamp when squared
    rows[13] = [(5, 1e-25), (8, 1e-25), (2, 3e-20)]
    rows[14] = [(3, 0.0)]
    rowptr = np.concatenate(([0], np.cumsum([len(r) for r in rows]))).astype(np.int32)
    flat = [t for r in rows for t in r]
    return rowptr, np.array([t[0] for t in flat], dtype=np.int32), np.array([t[1] for t in flat], dtype=F32)
