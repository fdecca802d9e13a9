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


def _check_candidates(candidates, V, S, starts, what, host_ptr=None, counts=None):
    """candidates: (M,) int64 strictly ascending vertex numbers of the union; S, starts: the checked per-mesh rounds and local
    starts.  Every mesh's start must be a candidate and its rounds at most its candidates (counts per mesh; one mesh: M)."""
    _check_index(candidates, V, what, 'candidates')
    M = int(candidates.numel())
    if M > 1 and not bool((candidates[1:] > candidates[:-1]).all()):
        raise ValueError(f'{what}: candidates must be strictly ascending vertex numbers (what a stored sample_idx is)')
    first = [0] * len(S) if host_ptr is None else host_ptr[:-1]
    counts = [M] if counts is None else counts
    cand = candidates.contiguous()
    where = torch.tensor([f + s for f, s in zip(first, starts)], dtype=torch.int64, device=cand.device)
    at = torch.searchsorted(cand, where).clamp(max=M - 1)
    found = (cand[at] == where).tolist()
    for b, (s, m) in enumerate(zip(S, counts)):
        of = '' if host_ptr is None else f' of mesh {b}'
        if not found[b]:
            raise ValueError(f'{what}: start{of} must be one of the candidates, got {starts[b]}')
        if s > m:
            raise ValueError(f'{what}: n_samples{of} must be at most its {m} candidates, got {s}')


def _fps(pos, face, pos_ptr, host_ptr, S, starts, graph, what, diagonals=False, candidates=None):
    """S, starts: per-mesh Python ints, checked; candidates: None or checked -> (idx (sum S,) int64 local, dist (V,), sweeps (B,)
    int64) on the device, and it"""
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
        if candidates is not None:
            mask = torch.zeros(V, dtype=torch.uint8, device=dev)
            mask[candidates.detach().to(dev)] = 1
            _lib.check(lib.fc_geodesic_fps_among(_ptr(ptr), _ptr(nbr), _ptr(length), V, int(nbr.numel()), _ptr(pp), B, max_range, _ptr(mask),
                                                 _ptr(tables[0]), _ptr(tables[1]), _ptr(tables[2]), out_ptr[-1], _ptr(idx), _ptr(dist),
                                                 _ptr(sweeps), _ptr(ws), nbytes, _stream()), 'fc_geodesic_fps_among')
            return idx, dist, sweeps
        _lib.check(lib.fc_geodesic_fps(_ptr(ptr), _ptr(nbr), _ptr(length), V, int(nbr.numel()), _ptr(pp), B, max_range, _ptr(tables[0]),
                                       _ptr(tables[1]), _ptr(tables[2]), out_ptr[-1], _ptr(idx), _ptr(dist), _ptr(sweeps), _ptr(ws), nbytes,
                                       _stream()), 'fc_geodesic_fps')
    return idx, dist, sweeps


def geodesic_farthest_point_sample(pos, face, n_samples, start=0, graph=None, return_dist=False, return_sweeps=False, diagonals=False,
                                   candidates=None):
    """(n_samples,) int64 vertex numbers in selection order.  idx[0] = start; idx[k+1] is the vertex not yet taken with the
    largest d_k, where d_k is the multi-source distance field of idx[:k+1] (the bits of nearest_sample(pos, face, idx[:k+1])[1]).
    +inf is the largest value, so another component, or a vertex in no face, is sampled before any reached vertex; ties go to
    the lowest vertex number; no vertex is taken twice, even where zero-length edges make d zero on vertices not taken.
    1 <= n_samples <= V, 0 <= start < V.  One launch: one workgroup runs all the rounds, each from the previous field.
    graph: mesh_edge_graph(pos, face), to build it once per mesh.  return_dist: also the final field d_{n_samples-1}, (V,)
    float32 (its maximum is the covering radius of the sample).  return_sweeps: also the relaxation sweeps summed over the
    rounds, a () int64 tensor.  diagonals: as in geodesic_distances (graph must then be None).
    candidates: None, or (M,) int64 STRICTLY ASCENDING vertex numbers (what a stored sample_idx is): only they may be taken.
    idx[k+1] is then the candidate not yet taken with the largest d_k, while d_k stays the field of idx[:k+1] over the WHOLE
    mesh -- every vertex relaxes, candidate or not -- with the same +inf and tie rules; with every vertex a candidate the result
    is the unrestricted one, index for index and bit for bit.  start must be a candidate and n_samples <= M."""
    what = 'geodesic_farthest_point_sample'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    S = _whole(n_samples, 1, V, what, 'n_samples', integral_floats=True)
    st = _whole(start, 0, V - 1, what, 'start', integral_floats=True)
    if candidates is not None:
        _check_candidates(candidates, V, [S], [st], what)
    idx, dist, sweeps = _fps(pos, face, None, None, [S], [st], graph, what, diagonals, candidates)
    out = (idx.to(pos.device),)
    if return_dist:
        out += (dist.to(pos.device),)
    if return_sweeps:
        out += (sweeps[0].to(pos.device),)
    return out if len(out) > 1 else out[0]


def geodesic_farthest_point_sample_batched(pos, face, pos_ptr, n_samples, start=0, graph=None, return_dist=False, return_sweeps=False,
                                           diagonals=False, candidates=None, candidates_ptr=None):
    """geodesic_farthest_point_sample for the B meshes of a union at once, one workgroup per mesh in one launch: mesh b is
    pos[pos_ptr[b]:pos_ptr[b+1]] (pos_ptr (B+1,) int64, host or device, checked on the host; face and graph are the union's),
    n_samples and start one integer for all meshes or one per mesh, 1 <= n_samples[b] <= n_b, 0 <= start[b] < n_b.  Returns the
    (sum n_samples,) int64 indices, mesh after mesh in selection order, each LOCAL to its mesh (add pos_ptr[b] for rows of pos),
    as farthest_point_sample_batched does: index for index what the single call gives for the mesh alone.
    return_dist: also the (V,) final fields; return_sweeps: also the (B,) int64 sweep totals.  diagonals: as in
    geodesic_distances (graph must then be None); none crosses meshes.
    candidates, candidates_ptr: both None, or as in geodesic_farthest_point_sample for every mesh at once: candidates (M,) int64
    strictly ascending vertex numbers of the UNION and candidates_ptr the (B+1,) int64 table of its ranges per mesh (a MeshBatch's
    sample_idx and ptr).  Every mesh needs at least one candidate, all of them inside its own vertex range; start[b] (local) must
    be one of them and n_samples[b] at most their number.  The results stay local to the mesh."""
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
    if (candidates is None) != (candidates_ptr is None):
        raise ValueError(f'{what}: candidates and candidates_ptr go together (the candidates of the union and their ranges per mesh): '
                         'give both or neither')
    if candidates is not None:
        _check_index(candidates, int(pos.shape[0]), what, 'candidates')
        hc = _batch_tables(pos_ptr, candidates_ptr, int(pos.shape[0]), int(candidates.numel()), what, 'candidates_ptr', candidates)[3]
        counts = [b - a for a, b in zip(hc, hc[1:])]
        if min(counts) < 1:
            raise ValueError(f'{what}: mesh {counts.index(min(counts))} has no candidates')
        _check_candidates(candidates, int(pos.shape[0]), S, st, what, host, counts)
    idx, dist, sweeps = _fps(pos, face, pos_ptr, host, S, st, graph, what, diagonals, candidates)
    out = (idx.to(pos.device),)
    if return_dist:
        out += (dist.to(pos.device),)
    if return_sweeps:
        out += (sweeps.to(pos.device),)
    return out if len(out) > 1 else out[0]


def geodesic_radius_edges(pos, face, sample_idx, epsilon, max_num_neighbors=512, pos_ptr=None, sample_ptr=None, graph=None,
                          return_dist=False, diagonals=False, queries=None):
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
    one synchronisation that sizes the output.  diagonals: as in geodesic_distances (graph must then be None).
    queries: None, or (Q,) int64 STRICTLY ASCENDING positions in sample_idx: only their balls are solved.  The result is exactly
    the rows of the unrestricted result whose column 0 is in queries, in the same order (return_dist alike); the neighbours j
    still run over every sample.  Q = 0 gives no rows and launches nothing."""
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
    Q = S          # the list slots the launches window: the queries given, else every sample
    if queries is not None:
        if not torch.is_tensor(queries) or queries.dim() != 1 or queries.dtype != torch.int64:
            raise ValueError(f'{what}: queries must be a 1-D int64 tensor, got '
                             f'{(tuple(queries.shape), queries.dtype) if torch.is_tensor(queries) else type(queries).__name__}')
        Q = int(queries.numel())
        if Q == 0:
            edges = torch.empty((0, 2), dtype=torch.int64, device=pos.device)
            return (edges, torch.empty(0, dtype=torch.float32, device=pos.device)) if return_dist else edges
        _check_index(queries, S, what, 'queries')
        if Q > 1 and not bool((queries[1:] > queries[:-1]).all()):
            raise ValueError(f'{what}: queries must be strictly ascending positions in sample_idx')
    p, _, (ptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    E_graph = int(nbr.numel())
    per_call, windows = _query_windows(Q, lib.fc_geodesic_ball_workspace_bytes(max_range, 1))          # (no slots up to LDS_VERTICES)
    with _on(dev):
        src = sample_idx.detach().to(dev).contiguous()
        pp, sp = tables_on(dev)
        nbytes = lib.fc_geodesic_ball_workspace_bytes(max_range, per_call)
        ws = _scratch(nbytes, dev, None)
        mesh = (_ptr(ptr), _ptr(nbr), _ptr(length), V, E_graph, _ptr(pp), _ptr(sp), B, max_range, _ptr(src), S)
        if queries is None:
            count_fn, fill_fn, names = lib.fc_geodesic_ball_count, lib.fc_geodesic_ball_fill, ('fc_geodesic_ball_count', 'fc_geodesic_ball_fill')
        else:          # the same launches over the list: count and off are indexed by the list slot
            qs = queries.detach().to(dev).contiguous()
            mesh += (_ptr(qs), Q)
            count_fn, fill_fn = lib.fc_geodesic_ball_count_at, lib.fc_geodesic_ball_fill_at
            names = ('fc_geodesic_ball_count_at', 'fc_geodesic_ball_fill_at')
        count = torch.empty(Q, dtype=torch.int32, device=dev)
        for q0, nq in windows:
            _lib.check(count_fn(*mesh, q0, nq, eps, K, _ptr(count), _ptr(ws), nbytes, _stream()), names[0])
        off = torch.zeros(Q + 1, dtype=torch.int64, device=dev)
        off[1:] = torch.cumsum(count, 0, dtype=torch.int64)
        E = int(off[-1])          # the one synchronisation: E sizes the output
        edges = torch.empty((E, 2), dtype=torch.int64, device=dev)
        dist = torch.empty(E, dtype=torch.float32, device=dev) if return_dist else None
        for q0, nq in windows:
            _lib.check(fill_fn(*mesh, q0, nq, eps, K, _ptr(off), E, _ptr(edges), _ptr(dist), _ptr(ws), nbytes, _stream()), names[1])
    return (edges.to(pos.device), dist.to(pos.device)) if return_dist else edges.to(pos.device)
