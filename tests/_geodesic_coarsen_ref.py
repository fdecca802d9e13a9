"""numpy float32 restatements of geodesic coarsening (csrc/fc_geodesic_fps.hip: fc_geodesic_fps_among, fc_geodesic_ball_*_at;
transforms.CoarsenSamples(sampling='geodesic')), built on _geodesic_ref and _geodesic_sampling_ref: farthest-point sampling
among candidates, ball edges of chosen queries, the coarse positions of a fine level, the folded strip on which Euclidean and
geodesic sampling differ, and the two figures compared there.  Uses nothing from the package."""
import numpy as np

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref

F32 = np.float32


def fps_among(ptr, nbr, length, candidates, n_samples, start, each_round=None):
    """sref.fps with `taken` preset on the vertices that are no candidates -> (idx (n_samples,) int64 in selection order, the
    final field (V,) float32 over ALL vertices).  each_round(k, idx[:k+1], d, free): the field after round k and the candidates
    still free."""
    V = len(ptr) - 1
    candidates = np.asarray(candidates, dtype=np.int64)
    assert 1 <= n_samples <= len(candidates) and start in candidates
    d = np.full(V, np.inf, dtype=F32)
    taken = np.ones(V, dtype=bool)
    taken[candidates] = False
    idx = []
    for k in range(n_samples):
        if k == 0:
            v = int(start)
        else:
            free = np.nonzero(~taken)[0]
            v = int(free[np.argmax(d[free])])          # (argmax: the first of the largest, and free ascends)
        taken[v] = True
        idx.append(v)
        sref._settle(ptr, nbr, length, d, v)
        if each_round is not None:
            each_round(k, np.array(idx, dtype=np.int64), d, np.nonzero(~taken)[0])
    return np.array(idx, dtype=np.int64), d


def mesh_fps_among(pos, face, candidates, n_samples, start):
    return fps_among(*gref.edge_graph(pos, face), candidates, n_samples, start)


def ball_edges_at(edges, dist, queries):
    """the rows of sref.ball_edges' result whose query is in `queries`, in the same order"""
    keep = np.isin(edges[:, 0], np.asarray(queries, dtype=np.int64))
    return edges[keep], dist[keep]


def coarsen_geodesic(ptr, nbr, length, sample_idx, n_coarse):
    """(S_c,) int64 ascending positions in sample_idx (ascending vertex numbers): geodesic sampling among the fine samples,
    started at the first of them, min(n_coarse, S_f) rounds"""
    sample_idx = np.asarray(sample_idx, dtype=np.int64)
    taken, _ = fps_among(ptr, nbr, length, sample_idx, min(n_coarse, len(sample_idx)), sample_idx[0])
    return np.sort(np.searchsorted(sample_idx, taken))


def folded_strip(nx, ny, h=0.125, gap=0.05):
    """gref.lattice(nx, ny, h) folded onto itself: with m = (nx - 1) // 2 and xm = m h, every vertex with x > xm moves to
    x' = 2 xm - x + h, z = gap.  Two flat sheets lie `gap` apart, joined by one column of sides of length `gap`: points that
    face each other across the gap are up to the strip's length apart on the surface."""
    pos, face = gref.lattice(nx, ny, h)
    xm = F32(((nx - 1) // 2) * h)
    far = pos[:, 0] > xm
    pos = pos.copy()
    pos[far, 0] = F32(2) * xm - pos[far, 0] + F32(h)
    pos[far, 2] = F32(gap)
    return pos, face


def euclidean_fps(points, n_samples, start=0):
    """the package's Euclidean rule: squared float32 distances ((dx*dx + dy*dy) + dz*dz), the running minimum, the largest next,
    ties to the lower index, no point twice -> (n_samples,) int64 in selection order"""
    points = np.asarray(points, dtype=F32)
    best = np.full(len(points), np.inf, dtype=F32)
    idx = [int(start)]
    for _ in range(n_samples - 1):
        d = points - points[idx[-1]]
        best = np.minimum(best, (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        best[idx[-1]] = -1          # (taken: below every distance)
        idx.append(int(np.argmax(best)))
    return np.array(idx, dtype=np.int64)


def covering_radius(ptr, nbr, length, fine, coarse_vertices):
    """the largest edge-graph distance from a fine sample (vertex numbers) to its nearest coarse sample"""
    return float(gref.dijkstra32(ptr, nbr, length, coarse_vertices)[np.asarray(fine)].max())
