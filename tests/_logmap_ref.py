"""numpy restatement of fieldconv_amd.logmap (csrc/fc_logmap.hip) and the meshes its tests share.  The distance field comes from
_geodesic_sampling_ref's bounded float32 Dijkstra, so the tree decisions (tight edges, hop counts, predecessors) use the same
bits as the device; the smooth part (frames, unfolding) runs in the dtype asked for: float32 in the device's order of
operations, or float64 as the yardstick of both.  Uses nothing from the package but, in closed_form, the closed-form sphere of
fieldconv_amd.data.synthetic that the icosphere case is measured against."""
import functools

import numpy as np

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref

F32 = np.float32


# ------------------------------------------------------------------ meshes
def icosphere(subdivisions):
    """unit icosphere: 12, 42, 162, 642 vertices for 0..3 subdivisions; outward-facing triangles"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1),
         (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8), (3, 9, 4),
         (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v).astype(F32), np.ascontiguousarray(np.array(f, dtype=np.int64).T)


def jittered_grid(nx, ny, h=0.125, seed=0):
    """gref.lattice in the plane z = 0 with every vertex moved by up to 0.3 h inside the plane (faces keep their orientation)"""
    pos, face = gref.lattice(nx, ny, h)
    rng = np.random.default_rng(seed)
    pos[:, :2] += (rng.random((nx * ny, 2)) * 0.6 - 0.3).astype(F32) * F32(h)
    return pos, face


def two_components():
    """sref.odd_mesh: two components, a vertex in no face, and vertex 47 a copy of vertex 14 joined to it by a (zero-area) face:
    a zero-length edge"""
    return sref.odd_mesh()


def frames_mesh():
    """a small surface, vertex 60 in no face, vertex 61 a copy of vertex 7 and a zero-area face (7, 61, 8) on the two"""
    pos, face = gref.surface(60, seed=2)
    pos = np.concatenate((pos, np.array([[3, 3, 3]], dtype=F32), pos[7:8]))
    return pos, np.ascontiguousarray(np.concatenate((face, np.array([[7], [61], [8]])), 1))


# ------------------------------------------------------------------ small vector algebra, every operation written out
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack((a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]), -1)


def frames(pos, face, dtype=F32):
    """(normal, e1, e2), each (V,3) of dtype: the corner-by-corner sum of the faces' cross products in ascending (face, corner)
    order -- per vertex that is ascending face order -- normalised; (0,0,1) where it vanishes"""
    p = pos.astype(dtype)
    V = p.shape[0]
    a, b, c = p[face[0]], p[face[1]], p[face[2]]
    cr = _cross(b - a, c - a)
    s = np.zeros((V, 3), dtype=dtype)
    for f in range(face.shape[1]):
        for k in range(3):
            s[face[k, f]] = s[face[k, f]] + cr[f]
    ln = np.sqrt(_dot(s, s))
    with np.errstate(divide='ignore', invalid='ignore'):
        n = np.where(ln[:, None] > 0, s / ln[:, None], np.array([0, 0, 1], dtype=dtype))
    ref = np.where(np.abs(n[:, 2:3]) < dtype(0.95), np.array([0, 0, 1], dtype=dtype), np.array([1, 0, 0], dtype=dtype))
    c1 = _cross(ref, n)
    e1 = c1 / np.sqrt(_dot(c1, c1))[:, None]
    e2 = _cross(n, e1)
    assert n.dtype == dtype and e1.dtype == dtype and e2.dtype == dtype
    return n, e1, e2


# ------------------------------------------------------------------ the tree: integer and bit decisions on the float32 field
def bounded_field(ptr, nbr, length, source, bound):
    d = np.full(len(ptr) - 1, np.inf, dtype=F32)
    sref._settle(ptr, nbr, length, d, source, bound=F32(bound))
    return d


def tree(ptr, nbr, length, d, source):
    """(h, pred) int64 (V,), -1 where there is none: breadth-first over the tight edges fl32(d[u] + len) == d[v] from the source
    gives the least fixpoint of h; pred[v] = the lowest-numbered tight u with h[u] = h[v] - 1"""
    V = len(ptr) - 1
    h = np.full(V, -1, dtype=np.int64)
    pred = np.full(V, -1, dtype=np.int64)
    h[source] = 0
    front = [int(source)]
    while front:
        nxt = []
        for u in front:
            e0, e1 = ptr[u], ptr[u + 1]
            vs = nbr[e0:e1]
            tight = np.isfinite(d[vs]) & ((d[u] + length[e0:e1]) == d[vs])
            for v in vs[tight]:
                if h[v] < 0:
                    h[v] = h[u] + 1
                    nxt.append(int(v))
        front = nxt
    for v in np.nonzero(h > 0)[0]:
        e0, e1 = ptr[v], ptr[v + 1]
        us = nbr[e0:e1]                                # ascending
        ok = np.isfinite(d[us]) & ((d[us] + length[e0:e1]) == d[v]) & (h[us] == h[v] - 1)
        pred[v] = us[ok][0]
    return h, pred


def edge_length_of(ptr, nbr, length, u, v):
    e0, e1 = ptr[v], ptr[v + 1]
    return length[e0 + np.searchsorted(nbr[e0:e1], u)]


# ------------------------------------------------------------------ the unfolding: smooth arithmetic in `dtype`
def child(pos, fr, u, v, ln, Lu, Xu, dtype):
    """the values (L, X) of the children v (K,) of the parents u (K,) over edges of length ln; complex as (K,2) arrays"""
    n, e1, e2 = fr
    one = dtype(1)
    w = pos[v] - pos[u]
    wn = _dot(w, n[u])
    tg = w - wn[:, None] * n[u]
    c1, c2 = _dot(tg, e1[u]), _dot(tg, e2[u])
    r = np.sqrt(c1 * c1 + c2 * c2)
    with np.errstate(divide='ignore', invalid='ignore'):
        s = ln.astype(dtype) / r
        c1, c2 = np.where(r > 0, c1 * s, dtype(0)), np.where(r > 0, c2 * s, dtype(0))
        cth = _dot(n[u], n[v])
        opc = one + cth
        k = _cross(n[u], n[v])
        ke = _cross(k, e1[u])
        f = _dot(k, e1[u]) / opc
        g_rot = (e1[u] * cth[:, None] + ke) + k * f[:, None]
        dn = _dot(e1[u], n[v])
        g_prj = e1[u] - dn[:, None] * n[v]
        g = np.where((opc > dtype(1e-6))[:, None], g_rot, g_prj)
        r1, r2 = _dot(g, e1[v]), _dot(g, e2[v])
        rn = np.sqrt(r1 * r1 + r2 * r2)
        r1, r2 = np.where(rn > 0, r1 / rn, one), np.where(rn > 0, r2 / rn, dtype(0))
    X = np.stack((r1 * Xu[:, 0] - r2 * Xu[:, 1], r1 * Xu[:, 1] + r2 * Xu[:, 0]), 1)
    L = np.stack((Lu[:, 0] + (Xu[:, 0] * c1 + Xu[:, 1] * c2), Lu[:, 1] + (Xu[:, 0] * c2 - Xu[:, 1] * c1)), 1)
    assert X.dtype == dtype and L.dtype == dtype
    return L, X


def chord(pos, s, t):
    """|p_t - p_s| in pos's dtype, in the order of the edge lengths"""
    d = pos[t] - pos[s]
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


class Case:
    """everything of one (mesh, samples, rows, bound) that does not depend on the dtype: the fields and the trees"""

    def __init__(self, pos, face, sample_idx, edges, bound, ranges=None):
        self.pos, self.face, self.sample_idx, self.edges, self.bound = pos, face, np.asarray(sample_idx), np.asarray(edges), bound
        self.graph = gref.edge_graph(pos, face)
        V, S = pos.shape[0], len(sample_idx)
        self.h = np.full((S, V), -1, dtype=np.int64)
        self.pred = np.full((S, V), -1, dtype=np.int64)
        for q in range(S):
            d = bounded_field(*self.graph, self.sample_idx[q], bound)
            self.h[q], self.pred[q] = tree(*self.graph, d, self.sample_idx[q])
        t = self.sample_idx[self.edges[:, 1]]
        self.reached = self.h[self.edges[:, 0], t] >= 0

    @functools.lru_cache(maxsize=None)
    def values(self, dtype):
        """(L (E,2), X (E,2)) of dtype for the rows"""
        ptr, nbr, length = self.graph
        pos = self.pos.astype(dtype)
        fr = frames(self.pos, self.face, dtype)
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
                # float32: the graph's own lengths, as on the device; float64: the length is part of the smooth arithmetic
                ln = np.array([edge_length_of(ptr, nbr, length, a, b) for a, b in zip(u, v)], dtype=F32) if dtype == F32 else chord(pos, u, v)
                L[v], X[v] = child(pos, fr, u, v, ln, L[u], X[u], dtype)
            mine = np.nonzero(self.edges[:, 0] == q)[0]
            t = self.sample_idx[self.edges[mine, 1]]
            Lr[mine], Xr[mine] = L[t], X[t]
            out = mine[h[t] < 0]                       # not reached: a child of the source over the chord
            if len(out):
                t = self.sample_idx[self.edges[out, 1]]
                sv = np.full(len(out), s)
                origin = np.zeros((len(out), 2), dtype=dtype)
                unit = np.stack((np.ones(len(out), dtype=dtype), np.zeros(len(out), dtype=dtype)), 1)
                Lr[out], Xr[out] = child(pos, fr, sv, t, chord(pos, sv, t), origin, unit, dtype)
        return Lr, Xr


def polar(L):
    """(logMag, logAng) of L (E,2) as the device forms them"""
    mag = np.sqrt(L[:, 0] * L[:, 0] + L[:, 1] * L[:, 1])
    ang = np.where((L[:, 0] == 0) & (L[:, 1] == 0), L.dtype.type(0), np.arctan2(L[:, 1], L[:, 0]))
    return mag, ang


def as_complex(a):
    return a[:, 0].astype(np.float64) + 1j * a[:, 1].astype(np.float64)


def all_pairs(S):
    a, b = np.meshgrid(np.arange(S), np.arange(S), indexing='ij')
    return np.stack((a.ravel(), b.ravel()), 1).astype(np.int64)


# ------------------------------------------------------------------ the icosphere case and the closed-form sphere
ICO_BOUND = 0.85          # about 20 of 128 samples inside a geodesic ball of the unit sphere (a cap of area 20 * 4 pi / 128)


@functools.lru_cache(maxsize=None)
def ico_case():
    pos, face = icosphere(3)
    samples = np.sort(sref.mesh_fps(pos, face, 128, 0)[0])
    edges, _ = sref.mesh_ball_edges(pos, face, samples, ICO_BOUND)
    return Case(pos, face, samples, edges, ICO_BOUND)


def closed_form(case):
    """synthetic's (dist, exp(i ang), exp(i xp_ang)) for the rows of an icosphere case"""
    from fieldconv_amd.data.synthetic import _edge_fields, _frames
    p = case.pos.astype(np.float64)
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    e1, e2 = _frames(p)
    s, t = case.sample_idx[case.edges[:, 0]], case.sample_idx[case.edges[:, 1]]
    dist, ang, xp_ang = _edge_fields(p[s], e1[s], e2[s], p[t], e1[t], e2[t])
    return dist, np.exp(1j * ang), np.exp(1j * xp_ang)


def closed_form_errors(case, L, X):
    """per-field maxima against the closed form: logMag relative, logAng and arg(xp) in radians (as angles between unit complex
    numbers: no branch cut), over the rows with distinct ends"""
    dist, ang, xp = closed_form(case)
    off = case.edges[:, 0] != case.edges[:, 1]
    Lc, Xc = as_complex(L), as_complex(X)
    mag = np.abs(np.abs(Lc[off]) - dist[off]) / dist[off]
    d_ang = np.abs(np.angle(Lc[off] / np.abs(Lc[off]) * np.conj(ang[off])))
    d_xp = np.abs(np.angle(Xc[off] / np.abs(Xc[off]) * np.conj(xp[off])))
    return float(mag.max()), float(d_ang.max()), float(d_xp.max())
