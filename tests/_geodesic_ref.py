"""numpy float32 restatements of fieldconv_amd.geodesic (csrc/fc_geodesic.hip) and the small meshes its tests share: the edge
graph, a heap Dijkstra with float32 additions, tight-edge labels, in-place randomly ordered sweeps, and the fixed-order
vertex masses and sample weights.  Uses nothing from the package."""
import heapq

import numpy as np

F32 = np.float32
NONE = np.iinfo(np.int32).max


# ------------------------------------------------------------------ meshes
def lattice(nx, ny, h=0.125):
    """nx x ny vertices with spacing h in the plane z = 0, every cell cut along the same diagonal -> pos (V,3), face (3,F)"""
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny), indexing='ij')
    pos = np.stack((ix.ravel() * h, iy.ravel() * h, np.zeros(nx * ny)), 1).astype(F32)
    v = lambda i, j: i * ny + j
    i, j = np.meshgrid(np.arange(nx - 1), np.arange(ny - 1), indexing='ij')
    i, j = i.ravel(), j.ravel()
    lower = np.stack((v(i, j), v(i + 1, j), v(i + 1, j + 1)))
    upper = np.stack((v(i, j), v(i + 1, j + 1), v(i, j + 1)))
    return pos, np.concatenate((lower, upper), 1).astype(np.int64)


def surface(n, seed=0):
    """n random points of the unit square, Delaunay-triangulated, lifted by a smooth height"""
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    face = Delaunay(xy).simplices.T.astype(np.int64)
    return np.concatenate((xy, z[:, None]), 1).astype(F32), np.ascontiguousarray(face)


def union(meshes):
    """disjoint union -> pos, face, pos_ptr"""
    ptr = np.cumsum([0] + [m[0].shape[0] for m in meshes])
    pos = np.concatenate([m[0] for m in meshes])
    face = np.concatenate([m[1] + o for m, o in zip(meshes, ptr[:-1])], 1)
    return pos, face, ptr.astype(np.int64)


def spread(V, n, seed=0):
    """n distinct vertices in a fixed pseudo-random order (not sorted: positions and vertex numbers differ)"""
    return np.random.default_rng(seed).permutation(V)[:n].astype(np.int64)


# ------------------------------------------------------------------ edge graph
def edge_graph(pos, face):
    """(ptr (V+1,) int64, nbr (E,) int64, length (E,) float32): the triangle sides in both directions without duplicates, by
    row, neighbours ascending; length = sqrt((dx*dx + dy*dy) + dz*dz), every operation a float32 operation"""
    V = pos.shape[0]
    a = np.concatenate((face[0], face[1], face[2], face[1], face[2], face[0]))
    b = np.concatenate((face[1], face[2], face[0], face[0], face[1], face[2]))
    key = np.unique(a * V + b)
    src, nbr = key // V, key % V
    keep = src != nbr
    src, nbr = src[keep], nbr[keep]
    ptr = np.searchsorted(src, np.arange(V + 1))
    d = pos[nbr] - pos[src]
    assert d.dtype == F32
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    assert length.dtype == F32
    return ptr, nbr, length


def slot_rows(ptr):
    return np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))


# ------------------------------------------------------------------ distances
def dijkstra32(ptr, nbr, length, sources):
    """heap Dijkstra whose every addition is a float32 addition -> (V,) float32, +inf where unreachable"""
    V = len(ptr) - 1
    d = np.full(V, np.inf, dtype=F32)
    heap = []
    for s in np.unique(sources):
        d[s] = 0
        heap.append((0.0, int(s)))
    heapq.heapify(heap)
    done = np.zeros(V, dtype=bool)
    while heap:
        dv, v = heapq.heappop(heap)
        if done[v] or dv > d[v]:
            continue
        done[v] = True
        e0, e1 = ptr[v], ptr[v + 1]
        cand = d[v] + length[e0:e1]                  # float32 + float32
        us = nbr[e0:e1]
        better = cand < d[us]
        for u, c in zip(us[better], cand[better]):
            d[u] = c
            heapq.heappush(heap, (float(c), int(u)))
    return d


def sweep_distances(ptr, nbr, length, sources, rng):
    """the same fixpoint by in-place pulls over the vertices in a fresh random order every sweep"""
    V = len(ptr) - 1
    d = np.full(V, np.inf, dtype=F32)
    d[np.asarray(sources)] = 0
    sweeps = 0
    while True:
        changed = False
        for v in rng.permutation(V):
            e0, e1 = ptr[v], ptr[v + 1]
            if e1 > e0:
                c = (d[nbr[e0:e1]] + length[e0:e1]).min()
                if c < d[v]:
                    d[v] = c
                    changed = True
        sweeps += 1
        if not changed:
            return d, sweeps


def _initial_labels(V, sources):
    label = np.full(V, NONE, dtype=np.int64)
    for q, s in enumerate(sources):
        if label[s] == NONE:
            label[s] = q
    return label


def tight_labels(ptr, nbr, length, d, sources, rng=None):
    """label[v] = the smallest position in `sources` that reaches v along tight edges fl32(d[u] + length) == d[v] (d[v]
    finite); -1 where none does.  In-place pulls over the vertices by ascending d (one pass settles everything but chains of
    zero-length edges) or, with rng, in a fresh random order every pass; passes are repeated until one changes nothing."""
    V = len(ptr) - 1
    label = _initial_labels(V, sources)
    by_d = np.argsort(d, kind='stable')
    while True:
        changed = False
        for v in (by_d if rng is None else rng.permutation(V)):
            if not np.isfinite(d[v]):
                continue
            e0, e1 = ptr[v], ptr[v + 1]
            us = nbr[e0:e1]
            tight = (d[us] + length[e0:e1]) == d[v]
            if tight.any():
                m = label[us[tight]].min()
                if m < label[v]:
                    label[v] = m
                    changed = True
        if not changed:
            break
    label[label == NONE] = -1
    return label


def nearest(pos, face, sources):
    """(label (V,) int64, dist (V,) float32) of one mesh"""
    ptr, nbr, length = edge_graph(pos, face)
    d = dijkstra32(ptr, nbr, length, sources)
    return tight_labels(ptr, nbr, length, d, sources), d


def rows(pos, face, sources):
    ptr, nbr, length = edge_graph(pos, face)
    return np.stack([dijkstra32(ptr, nbr, length, [s]) for s in sources])


def tied_vertices(ptr, nbr, length, d, label):
    """vertices with two tight predecessors that carry different labels"""
    out = []
    for v in range(len(ptr) - 1):
        if not np.isfinite(d[v]) or d[v] == 0:
            continue
        e0, e1 = ptr[v], ptr[v + 1]
        us = nbr[e0:e1]
        tight = (d[us] + length[e0:e1]) == d[v]
        if len(set(label[us[tight]])) > 1:
            out.append(v)
    return out


# ------------------------------------------------------------------ masses and weights
def face_areas(pos, face):
    a, b, c = pos[face[0]], pos[face[1]], pos[face[2]]
    u, w = b - a, c - a
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = F32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
    assert area.dtype == F32
    return area


def ordered_sums(values, keys, K):
    """out[k] = the values with key k added in float32 in their order of appearance (keys < 0: nowhere)"""
    out = np.zeros(K, dtype=F32)
    for x, k in zip(values, keys):
        if k >= 0:
            out[k] = out[k] + x
    return out


def vertex_masses(pos, face):
    area = face_areas(pos, face)
    return ordered_sums(np.tile(area, 3), face.reshape(-1), pos.shape[0]) / F32(3)


def sample_weights(pos, face, label, S):
    return ordered_sums(vertex_masses(pos, face), label, S)[:, None]


def area64(pos, face):
    p = pos.astype(np.float64)
    a, b, c = p[face[0]], p[face[1]], p[face[2]]
    return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())
