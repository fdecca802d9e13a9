"""numpy float32 restatements of fieldconv_amd.geodesic_sampling (csrc/fc_geodesic_fps.hip), built on _geodesic_ref: geodesic
farthest-point sampling by an incremental pruned Dijkstra, and geodesic-ball support edges from unbounded Dijkstra rows (and,
to show the bound changes nothing, from a bounded one).  Uses nothing from the package."""
import heapq

import numpy as np

import _geodesic_ref as gref

F32 = np.float32


def _settle(ptr, nbr, length, d, source, bound=None):
    """d[source] = 0 and a heap Dijkstra from it that only ever lowers d (float32 additions): the incremental step.  With a
    bound, candidates must be < bound."""
    d[source] = 0
    heap = [(0.0, int(source))]
    while heap:
        dv, v = heapq.heappop(heap)
        if dv > d[v]:
            continue
        e0, e1 = ptr[v], ptr[v + 1]
        cand = d[v] + length[e0:e1]                  # float32 + float32
        us = nbr[e0:e1]
        better = cand < d[us]
        if bound is not None:
            better &= cand < bound
        for u, c in zip(us[better], cand[better]):
            d[u] = c
            heapq.heappush(heap, (float(c), int(u)))


def fps(ptr, nbr, length, n_samples, start=0, each_round=None):
    """-> (idx (n_samples,) int64 in selection order, the final field (V,) float32).  idx[0] = start; the next sample is the
    vertex not yet taken with the largest d (+inf the largest of all), ties to the lowest vertex number.
    each_round(k, idx[:k+1], d) is called with the field after every round."""
    V = len(ptr) - 1
    assert 1 <= n_samples <= V and 0 <= start < V
    d = np.full(V, np.inf, dtype=F32)
    taken = np.zeros(V, dtype=bool)
    idx = []
    for k in range(n_samples):
        if k == 0:
            v = start
        else:
            free = np.nonzero(~taken)[0]
            v = int(free[np.argmax(d[free])])          # (argmax: the first of the largest, and free ascends)
        taken[v] = True
        idx.append(v)
        _settle(ptr, nbr, length, d, v)
        if each_round is not None:
            each_round(k, np.array(idx, dtype=np.int64), d)
    return np.array(idx, dtype=np.int64), d


def mesh_fps(pos, face, n_samples, start=0):
    return fps(*gref.edge_graph(pos, face), n_samples, start)


def _rows_to_edges(rows, sample_idx, epsilon, max_num_neighbors, ranges):
    """rows[q]: the field of sample q over the vertices -> (edges (E,2) int64, dist (E,) float32)"""
    eps = F32(epsilon)
    S = len(sample_idx)
    ranges = [(0, S)] if ranges is None else ranges
    edges, dist = [], []
    for s0, s1 in ranges:
        for q in range(s0, s1):
            dq = rows[q][sample_idx[s0:s1]]
            js = np.nonzero(dq < eps)[0]                                    # strict
            if len(js) > max_num_neighbors:
                order = np.lexsort((js, dq[js]))                            # by distance, then position
                js = np.sort(js[order[:max_num_neighbors]])
            edges += [(q, s0 + j) for j in js]
            dist += [dq[j] for j in js]
    return np.array(edges, dtype=np.int64).reshape(-1, 2), np.array(dist, dtype=F32)


def ball_edges(ptr, nbr, length, sample_idx, epsilon, max_num_neighbors=512, sample_ranges=None, bounded=False):
    """rows [q, j] (positions in sample_idx) with d_q[sample_idx[j]] < float32(epsilon), q ascending, j ascending; more than
    max_num_neighbors: the nearest by (distance, position).  sample_ranges: [(s0, s1), ...] position ranges that search among
    themselves only (the meshes of a union; their vertices are not connected anyway, this only scopes the positions).
    bounded: the rows come from a Dijkstra that accepts only candidates < epsilon, not from the unbounded dijkstra32."""
    V = len(ptr) - 1
    rows = []
    for s in sample_idx:
        if bounded:
            d = np.full(V, np.inf, dtype=F32)
            _settle(ptr, nbr, length, d, s, bound=F32(epsilon))
        else:
            d = gref.dijkstra32(ptr, nbr, length, [s])
        rows.append(d)
    return _rows_to_edges(rows, np.asarray(sample_idx), epsilon, max_num_neighbors, sample_ranges)


def mesh_ball_edges(pos, face, sample_idx, epsilon, max_num_neighbors=512, sample_ranges=None):
    return ball_edges(*gref.edge_graph(pos, face), sample_idx, epsilon, max_num_neighbors, sample_ranges)


def odd_mesh():
    """two components (30 and 16 vertices), vertex 46 in no face, vertex 47 a copy of vertex 14 joined to it by a face: a
    zero-length edge"""
    pos, face, _ = gref.union([gref.lattice(5, 6), gref.lattice(4, 4)])
    pos = np.concatenate((pos, np.array([[9, 9, 9]], dtype=F32), pos[14:15]))
    face = np.concatenate((face, np.array([[14], [47], [15]])), 1)
    return pos, face
