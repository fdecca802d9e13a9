"""numpy float32 restatement of fieldconv_amd.geodesic.mesh_edge_graph(pos, face, diagonals=True) (csrc/fc_mesh_graph.hip): the
triangle sides of _geodesic_ref.edge_graph plus the unfolded diagonals, in plain loops and the kernels' order of operations; the
hand-made meshes its tests share; and the log-map case of _logmap_ref on a graph handed in.  Uses nothing from the package."""
import functools

import numpy as np

import _geodesic_ref as gref
import _logmap_ref as lref

F32 = np.float32


# ------------------------------------------------------------------ the unfolding
def unfold(pos, u, v, c, d, dtype=F32):
    """the length of the diagonal {c, d} across the side (u, v), u < v, c from the lower-numbered face; None where there is
    none.  Scalars of `dtype`, every operation rounded on its own."""
    p = pos.astype(dtype)
    zero = dtype(0)
    e = p[v] - p[u]
    L2 = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    if L2 == zero:
        return None
    L = np.sqrt(L2)
    xy = []
    for w in (c, d):
        r = p[w] - p[u]
        x = ((r[0] * e[0] + r[1] * e[1]) + r[2] * e[2]) / L
        h2 = ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) - x * x
        xy.append((x, np.sqrt(h2 if h2 > zero else zero)))
    (xc, yc), (xd, yd) = xy
    s = yc + yd
    if s <= zero:
        return None
    t = xc + (xd - xc) * (yc / s)
    if not (zero < t and t < L):
        return None
    ln = np.sqrt((xc - xd) * (xc - xd) + s * s)
    assert ln.dtype == dtype
    return ln


def candidates(pos, face):
    """[(min(c,d), max(c,d), length float32, length float64)] in ascending order of the side (u, v) they cross.  The decisions
    are float32's; the float64 length of the same unfolding rides along as the yardstick of the smooth arithmetic."""
    runs = {}
    for f in range(face.shape[1]):
        a, b, c = (int(x) for x in face[:, f])
        if a == b or b == c or c == a:
            continue                                  # a face that names a vertex twice counts for no side
        for x, y, o in ((a, b, c), (b, c, a), (c, a, b)):
            runs.setdefault((min(x, y), max(x, y)), []).append(o)          # faces ascend: the lower-numbered face comes first
    out = []
    for (u, v) in sorted(runs):
        opposite = runs[(u, v)]
        if len(opposite) != 2 or opposite[0] == opposite[1]:
            continue                                  # boundary, non-manifold, or one face listed twice
        c, d = opposite
        ln = unfold(pos, u, v, c, d)
        if ln is not None:
            ln64 = unfold(pos, u, v, c, d, np.float64)
            out.append((min(c, d), max(c, d), ln, np.float64(ln) if ln64 is None else ln64))
    return out


def edge_graph(pos, face, with_float64=False):
    """(ptr (V+1,) int64, nbr (E,) int64, length (E,) float32) in gref.edge_graph's layout: sides and diagonals, both directions
    of every pair, by row with neighbours ascending; a pair that arises more than once keeps the smallest float32 length.
    with_float64: also (E,) float64, the float64 length of whichever entry won (a side: the float64 chord)."""
    sptr, snbr, slen = gref.edge_graph(pos, face)
    p64 = pos.astype(np.float64)
    best = {}
    for u, v, ln in zip(gref.slot_rows(sptr), snbr, slen):
        best[(int(u), int(v))] = (ln, np.linalg.norm(p64[v] - p64[u]))
    for lo, hi, ln, ln64 in candidates(pos, face):
        for pair in ((lo, hi), (hi, lo)):
            if pair not in best or ln < best[pair][0]:
                best[pair] = (ln, ln64)
    pairs = sorted(best)
    V = pos.shape[0]
    src = np.array([p[0] for p in pairs], dtype=np.int64)
    nbr = np.array([p[1] for p in pairs], dtype=np.int64)
    length = np.array([best[p][0] for p in pairs], dtype=F32)
    ptr = np.searchsorted(src, np.arange(V + 1))
    if with_float64:
        return ptr, nbr, length, np.array([best[p][1] for p in pairs], dtype=np.float64)
    return ptr, nbr, length


def pairs_of(ptr, nbr, length):
    """{(u, v): length} over the directed slots"""
    return {(int(u), int(v)): l for u, v, l in zip(gref.slot_rows(ptr), nbr, length)}


# ------------------------------------------------------------------ hand-made meshes
def _mesh(points, faces):
    return np.array(points, dtype=F32), np.ascontiguousarray(np.array(faces, dtype=np.int64).T.reshape(3, -1))


def square():
    """the unit square cut along 0-2: gains the diagonal 1-3 of length fl32(sqrt(2))"""
    return _mesh([(0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)], [(0, 1, 2), (0, 2, 3)])


def concave():
    """a dart with its reflex vertex 2, cut along 0-2: the segment 1-3 passes outside, beyond vertex 2 (t = 2 > L = 1)"""
    return _mesh([(0, 0, 0), (2, -1, 0), (1, 0, 0), (2, 1, 0)], [(0, 1, 2), (0, 2, 3)])


def single():
    """one triangle: boundary sides only"""
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2)])


def fan3():
    """three faces on the side 0-1 (non-manifold); every other side is a boundary"""
    return _mesh([(0, 0, 0), (1, 0, 0), (0.5, 1, 0), (0.5, -1, 0), (0.5, 0, 1)], [(0, 1, 2), (1, 0, 3), (0, 1, 4)])


def twice():
    """one face listed twice: every side has two faces, with c == d"""
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2), (0, 1, 2)])


def degenerate():
    """a triangle and the face (0, 1, 1) on its side 0-1: counted, that face would make 0-1 a side of two faces"""
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 1, 0)], [(0, 1, 2), (0, 1, 1)])


def square_with_degenerate():
    """the square with a third face (0, 2, 2) on its cut: that face counts for nothing, so the cut keeps its two faces"""
    pos, face = square()
    return pos, np.ascontiguousarray(np.concatenate((face, np.array([[0], [2], [2]])), 1))


def zero_side():
    """vertex 2 is a copy of vertex 0 and the two faces share the side 0-2 of length zero"""
    return _mesh([(0, 0, 0), (1, 0, 0), (0, 0, 0), (0, 1, 0)], [(0, 1, 2), (0, 2, 3)])


def octahedron():
    """apexes 0 and 1 over an irregular equator 2, 3, 4, 5: each of the four equator sides unfolds to the pair {0, 1}, which is
    no side, with four different lengths; and each pair of opposite equator vertices arises from two sides of each apex"""
    return _mesh([(0, 0, 0.3), (0, 0, -0.2), (1, 0, 0), (0, 1.3, 0), (-0.8, 0, 0), (0, -0.9, 0)],
                 [(0, 2, 3), (0, 3, 4), (0, 4, 5), (0, 5, 2), (1, 3, 2), (1, 4, 3), (1, 5, 4), (1, 2, 5)])


HAND_MADE = (square, concave, single, fan3, twice, degenerate, square_with_degenerate, zero_side, octahedron)


def joined():
    """the hand-made meshes as one mesh (disjoint union)"""
    return gref.union([m() for m in HAND_MADE])


# ------------------------------------------------------------------ accuracy against the unit sphere
def sphere_accuracy(pos, ptr, nbr, length, min_true=0.2):
    """(mean, max) of d / true over the pairs (source, vertex) further than min_true apart: float64 Dijkstra over the graph's
    lengths against the great-circle distance; sources are the 41 vertices arange(0, V, V // 40)"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra
    V = pos.shape[0]
    p = pos.astype(np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    sources = np.arange(0, V, V // 40)
    d = dijkstra(csr_matrix((length.astype(np.float64), nbr, ptr), shape=(V, V)), directed=True, indices=sources)
    true = np.arccos(np.clip(p[sources] @ p.T, -1.0, 1.0))
    far = true > min_true
    ratio = d[far] / true[far]
    return float(ratio.mean()), float(ratio.max())


# ------------------------------------------------------------------ the log map on a graph handed in
class GraphCase(lref.Case):
    """lref.Case on the enriched graph: the same trees and unfolding, the graph's lengths in float32 and, as the float64
    yardstick, the float64 unfolded length of every edge (for a side that is the chord lref.Case takes)"""

    def __init__(self, pos, face, sample_idx, edges, bound):
        self.pos, self.face, self.sample_idx, self.edges, self.bound = pos, face, np.asarray(sample_idx), np.asarray(edges), bound
        ptr, nbr, length, self.length64 = edge_graph(pos, face, with_float64=True)
        self.graph = (ptr, nbr, length)
        V, S = pos.shape[0], len(sample_idx)
        self.h = np.full((S, V), -1, dtype=np.int64)
        self.pred = np.full((S, V), -1, dtype=np.int64)
        for q in range(S):
            d = lref.bounded_field(*self.graph, self.sample_idx[q], bound)
            self.h[q], self.pred[q] = lref.tree(*self.graph, d, self.sample_idx[q])
        t = self.sample_idx[self.edges[:, 1]]
        self.reached = self.h[self.edges[:, 0], t] >= 0

    @functools.lru_cache(maxsize=None)
    def values(self, dtype):
        """(L (E,2), X (E,2)) of dtype for the rows"""
        ptr, nbr, length = self.graph
        lengths = length if dtype == F32 else self.length64
        pos = self.pos.astype(dtype)
        fr = lref.frames(self.pos, self.face, dtype)
        E = len(self.edges)
        Lr, Xr = np.zeros((E, 2), dtype=dtype), np.zeros((E, 2), dtype=dtype)
        for q in np.unique(self.edges[:, 0]):
            s = self.sample_idx[q]
            h, pred = self.h[q], self.pred[q]
            L, X = np.zeros((len(h), 2), dtype=dtype), np.zeros((len(h), 2), dtype=dtype)
            X[s, 0] = 1
            for level in range(1, h.max() + 1):
                v = np.nonzero(h == level)[0]
                u = pred[v]
                ln = np.array([lref.edge_length_of(ptr, nbr, lengths, a, b) for a, b in zip(u, v)], dtype=dtype)
                L[v], X[v] = lref.child(pos, fr, u, v, ln, L[u], X[u], dtype)
            mine = np.nonzero(self.edges[:, 0] == q)[0]
            t = self.sample_idx[self.edges[mine, 1]]
            Lr[mine], Xr[mine] = L[t], X[t]
            out = mine[h[t] < 0]                       # not reached: a child of the source over the chord
            if len(out):
                t = self.sample_idx[self.edges[out, 1]]
                sv = np.full(len(out), s)
                origin = np.zeros((len(out), 2), dtype=dtype)
                unit = np.stack((np.ones(len(out), dtype=dtype), np.zeros(len(out), dtype=dtype)), 1)
                Lr[out], Xr[out] = lref.child(pos, fr, sv, t, lref.chord(pos, sv, t), origin, unit, dtype)
        return Lr, Xr
