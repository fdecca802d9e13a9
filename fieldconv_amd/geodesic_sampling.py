"""Sampling and neighbourhoods by the mesh's own metric (csrc/fc_geodesic_fps.hip): farthest-point sampling and epsilon-ball
support edges over the edge-graph distances of fieldconv_amd.geodesic -- the intrinsic counterparts of
transforms.farthest_point_sample and transforms.radius_edges, which measure through the ambient space and so join vertices
across a gap (a hand near a thigh) that are far apart on the surface.

Everything is defined through least fixpoints of d[source] = 0, d[v] = min_u fl32(d[u] + length(u,v)) over mesh_edge_graph's
CSR, so results are exact and restatable (tests/_geodesic_sampling_ref.py): the same bits on every run, whatever the schedule.

Conventions are those of geodesic.py: pos (V,3) float32, face (3,F) int64, on a ROCm device or on the host; the arithmetic
runs on the device either way and results go back to pos's device.  There is no CPU arithmetic path.  Bad arguments raise
ValueError before anything is launched.  Nothing here is differentiable."""
import torch

from . import _lib
from .geodesic import LDS_VERTICES          # noqa: F401  (the family's one LDS capacity, readable from here as well)
from ._launch import on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .geodesic import _batch_tables, _check_diagonals, _check_index, _check_mesh, _prepare, _query_windows
from .pooling import check_ptr, per_mesh, ptr_on


def _fps(pos, face, pos_ptr, host_ptr, S, starts, graph, what, diagonals=False):
    """S, starts: per-mesh Python ints, checked -> (idx (sum S,) int64 local, dist (V,), sweeps (B,) int64) on the device, and it"""
    V = int(pos.shape[0])
    B = len(S)
    max_range = V if host_ptr is None else max(b - a for a, b in zip(host_ptr, host_ptr[1:]))
    p, _, (ptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    out_ptr = [0]
    for s in S:
        out_ptr.append(out_ptr[-1] + s)
    with _on(dev):
        tables = torch.tensor([S, starts, out_ptr[:-1]], dtype=torch.int64).to(dev)
        pp = None if host_ptr is None else ptr_on(pos_ptr, host_ptr, dev)
        nbytes = lib.fc_geodesic_fps_workspace_bytes(V, max_range)
        ws = _scratch(nbytes, dev, None)
        idx = torch.empty(out_ptr[-1], dtype=torch.int64, device=dev)
        dist = torch.empty(V, dtype=torch.float32, device=dev)
        sweeps = torch.empty(B, dtype=torch.int64, device=dev)
        _lib.check(lib.fc_geodesic_fps(_ptr(ptr), _ptr(nbr), _ptr(length), V, int(nbr.numel()), _ptr(pp), B, max_range, _ptr(tables[0]),
                                       _ptr(tables[1]), _ptr(tables[2]), out_ptr[-1], _ptr(idx), _ptr(dist), _ptr(sweeps), _ptr(ws), nbytes,
                                       _stream()), 'fc_geodesic_fps')
    return idx, dist, sweeps


def geodesic_farthest_point_sample(pos, face, n_samples, start=0, graph=None, return_dist=False, return_sweeps=False, diagonals=False):
    """(n_samples,) int64 vertex numbers in selection order.  idx[0] = start; idx[k+1] is the vertex not yet taken with the
    largest d_k, where d_k is the multi-source distance field of idx[:k+1] (the bits of nearest_sample(pos, face, idx[:k+1])[1]).
    +inf is the largest value, so another component, or a vertex in no face, is sampled before any reached vertex; ties go to
    the lowest vertex number; no vertex is taken twice, even where zero-length edges make d zero on vertices not taken.
    1 <= n_samples <= V, 0 <= start < V.  One launch: one workgroup runs all the rounds, each from the previous field.
    graph: mesh_edge_graph(pos, face), to build it once per mesh.  return_dist: also the final field d_{n_samples-1}, (V,)
    float32 (its maximum is the covering radius of the sample).  return_sweeps: also the relaxation sweeps summed over the
    rounds, a () int64 tensor.  diagonals: as in geodesic_distances (graph must then be None)."""
    what = 'geodesic_farthest_point_sample'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    S = _whole(n_samples, 1, V, what, 'n_samples', integral_floats=True)
    st = _whole(start, 0, V - 1, what, 'start', integral_floats=True)
    idx, dist, sweeps = _fps(pos, face, None, None, [S], [st], graph, what, diagonals)
    out = (idx.to(pos.device),)
    if return_dist:
        out += (dist.to(pos.device),)
    if return_sweeps:
        out += (sweeps[0].to(pos.device),)
    return out if len(out) > 1 else out[0]


def geodesic_farthest_point_sample_batched(pos, face, pos_ptr, n_samples, start=0, graph=None, return_dist=False, return_sweeps=False,
                                           diagonals=False):
    """geodesic_farthest_point_sample for the B meshes of a union at once, one workgroup per mesh in one launch: mesh b is
    pos[pos_ptr[b]:pos_ptr[b+1]] (pos_ptr (B+1,) int64, host or device, checked on the host; face and graph are the union's),
    n_samples and start one integer for all meshes or one per mesh, 1 <= n_samples[b] <= n_b, 0 <= start[b] < n_b.  Returns the
    (sum n_samples,) int64 indices, mesh after mesh in selection order, each LOCAL to its mesh (add pos_ptr[b] for rows of pos),
    as farthest_point_sample_batched does: index for index what the single call gives for the mesh alone.
    return_dist: also the (V,) final fields; return_sweeps: also the (B,) int64 sweep totals.  diagonals: as in
    geodesic_distances (graph must then be None); none crosses meshes."""
    what = 'geodesic_farthest_point_sample_batched'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    host = check_ptr(pos_ptr, int(pos.shape[0]), what, 'pos_ptr')
    B = len(host) - 1
    S, st = per_mesh(n_samples, B, what, 'n_samples'), per_mesh(start, B, what, 'start')
    for b in range(B):
        n_b = host[b + 1] - host[b]
        if n_b < 1:
            raise ValueError(f'{what}: mesh {b} holds no vertices')
        S[b] = _whole(S[b], 1, n_b, what, 'n_samples', f' of mesh {b}', integral_floats=True)
        st[b] = _whole(st[b], 0, n_b - 1, what, 'start', f' of mesh {b}', integral_floats=True)
    idx, dist, sweeps = _fps(pos, face, pos_ptr, host, S, st, graph, what, diagonals)
    out = (idx.to(pos.device),)
    if return_dist:
        out += (dist.to(pos.device),)
    if return_sweeps:
        out += (sweeps.to(pos.device),)
    return out if len(out) > 1 else out[0]


def geodesic_radius_edges(pos, face, sample_idx, epsilon, max_num_neighbors=512, pos_ptr=None, sample_ptr=None, graph=None,
                          return_dist=False, diagonals=False):
    """(E,2) int64 rows [q, j], POSITIONS in sample_idx: one row for every pair with d_q[sample_idx[j]] < fl32(epsilon), where
    d_q is the single-source distance field of vertex sample_idx[q] (row q of geodesic_distances(pos, face, sample_idx)).
    The comparison is strict and q is its own neighbour.  Rows are grouped by q ascending, j ascending inside a group: the
    layout of radius_edges.  A query with more than max_num_neighbors such samples keeps the nearest by (distance, position).
    sample_idx (S,) int64 must be STRICTLY ASCENDING (what SupportGraph stores).  return_dist: also the (E,) float32 distances.
    The relation can be asymmetric in the last bit at the threshold: d_q[j] and d_j[q] add the same lengths in opposite order,
    so one may round below epsilon and the other onto it.
    pos_ptr, sample_ptr: both None, or the (B+1,) int64 range tables of a MeshBatch (batch.pos_ptr, batch.ptr): a query searches
    its own mesh only, and a batch of small meshes stays in LDS although their union would not.
    One workgroup per query relaxes only while candidates stay below epsilon: a prefix of a shortest path is never longer than
    the path, so every distance below epsilon is the unbounded one.  The queries are solved twice (count, then fill) around the
    one synchronisation that sizes the output.  diagonals: as in geodesic_distances (graph must then be None)."""
    from .transforms.support_graph import _check_epsilon, _check_k
    what = 'geodesic_radius_edges'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    S = int(sample_idx.numel())
    if S > 1 and not bool((sample_idx[1:] > sample_idx[:-1]).all()):
        raise ValueError(f'{what}: sample_idx must be strictly ascending (sort it: positions then follow the vertex numbers)')
    eps = _check_epsilon(epsilon, what)
    K = _check_k(max_num_neighbors, what)
    if K > 2 ** 31 - 1:
        raise ValueError(f'{what}: max_num_neighbors must stay below 2^31')
    B, max_range, _, _, tables_on = _batch_tables(pos_ptr, sample_ptr, V, S, what, 'sample_ptr', sample_idx)
    p, _, (ptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    E_graph = int(nbr.numel())
    per_call, windows = _query_windows(S, lib.fc_geodesic_ball_workspace_bytes(max_range, 1))          # (no slots up to LDS_VERTICES)
    with _on(dev):
        src = sample_idx.detach().to(dev).contiguous()
        pp, sp = tables_on(dev)
        nbytes = lib.fc_geodesic_ball_workspace_bytes(max_range, per_call)
        ws = _scratch(nbytes, dev, None)
        count = torch.empty(S, dtype=torch.int32, device=dev)
        for q0, nq in windows:
            _lib.check(lib.fc_geodesic_ball_count(_ptr(ptr), _ptr(nbr), _ptr(length), V, E_graph, _ptr(pp), _ptr(sp), B, max_range, _ptr(src),
                                                  S, q0, nq, eps, K, _ptr(count), _ptr(ws), nbytes, _stream()),
                       'fc_geodesic_ball_count')
        off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        E = int(off[-1])          # the one synchronisation: E sizes the output
        edges = torch.empty((E, 2), dtype=torch.int64, device=dev)
        dist = torch.empty(E, dtype=torch.float32, device=dev) if return_dist else None
        for q0, nq in windows:
            _lib.check(lib.fc_geodesic_ball_fill(_ptr(ptr), _ptr(nbr), _ptr(length), V, E_graph, _ptr(pp), _ptr(sp), B, max_range, _ptr(src),
                                                 S, q0, nq, eps, K, _ptr(off), E, _ptr(edges), _ptr(dist), _ptr(ws),
                                                 nbytes, _stream()), 'fc_geodesic_ball_fill')
    return (edges.to(pos.device), dist.to(pos.device)) if return_dist else edges.to(pos.device)
