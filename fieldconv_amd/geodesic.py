"""Mesh geodesics on the device (csrc/fc_geodesic.hip): shortest paths over the mesh's edge graph, from one source or many.

This is the EDGE-GRAPH metric, not the heat method the reference's fcutils solves: paths run along triangle sides, so a
distance overestimates the true geodesic -- by 6 to 7 % on average and up to 23 % on a sphere, however fine the mesh; with the
unfolded diagonals of mesh_edge_graph(..., diagonals=True) by about 1 % on average and up to 5 % -- and nearest-sample cells
agree with the true ones except near cell boundaries.  What it buys: the result is deterministic and restatable bit for bit (a heap
Dijkstra with float32 additions gives the same numbers, tests/_geodesic_ref.py), as FPS and the radius search are.

pos (V,3) float32, face (3,F) int64 (the PyG layout), on a ROCm device or on the host: the arithmetic runs on the device
either way and results go back to pos's device, as in transforms.SupportGraph.  There is no CPU arithmetic path.  Bad
arguments raise ValueError before anything is launched.  Nothing here is differentiable."""
import torch

from . import _lib
from ._launch import device_of as _device_of, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .pooling import check_ptr, ptr_on

# Vertices of one mesh solved in LDS by every solver of the family (fc_geodesic_lds_vertices: 8 B per vertex of the CU's 160 KiB
# for distances and labels, 7 B for sampling, 6 B for a ball); a larger mesh runs the same loops in global memory, still one
# workgroup per problem.
LDS_VERTICES = 20000
_ROW_CHUNK_FLOATS = 1 << 26          # distance rows per launch: at most 256 MiB of them
_WORKSPACE_BYTES = 1 << 28           # queries per launch where they need workspace slots: at most 256 MiB of them


def _check_mesh(pos, face, what):
    if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[1] != 3 or pos.shape[0] < 1:
        raise ValueError(f'{what}: pos must be a (V,3) tensor with V >= 1, got {tuple(pos.shape) if torch.is_tensor(pos) else type(pos).__name__}')
    if pos.dtype != torch.float32:
        raise ValueError(f'{what}: pos must be float32, got {pos.dtype}')
    if not torch.is_tensor(face) or face.dim() != 2 or face.shape[0] != 3 or face.dtype != torch.int64:
        raise ValueError(f'{what}: face must be a (3,F) int64 tensor, got '
                         f'{(tuple(face.shape), face.dtype) if torch.is_tensor(face) else type(face).__name__}')
    if pos.shape[0] > 2 ** 31 - 1 or 6 * face.shape[1] > 2 ** 31 - 1:
        raise ValueError(f'{what}: vertices and directed edges (6 per face) are 32-bit indices in the kernels: at most 2^31 - 1 of each')


def _check_index(idx, n, what, name):
    """(K,) int64 with K >= 1 and every value in [0,n) (one synchronisation) -> the tensor"""
    if not torch.is_tensor(idx) or idx.dim() != 1 or idx.dtype != torch.int64:
        raise ValueError(f'{what}: {name} must be a 1-D int64 tensor, got {(tuple(idx.shape), idx.dtype) if torch.is_tensor(idx) else type(idx).__name__}')
    if idx.numel() < 1:
        raise ValueError(f'{what}: {name} is empty')
    lo, hi = int(idx.min()), int(idx.max())
    if lo < 0 or hi >= n:
        raise ValueError(f'{what}: {name} must lie in [0, {n}), got values from {lo} to {hi}')
    return idx


def _face_on(face, V, dev, what):
    f = face.detach().to(dev).contiguous()
    if f.shape[1] and (int(f.min()) < 0 or int(f.max()) >= V):
        raise ValueError(f'{what}: face refers to a vertex outside [0, {V})')
    return f


def _graph_on(graph, V, dev, what):
    if not isinstance(graph, (tuple, list)) or len(graph) != 3 or not all(torch.is_tensor(t) for t in graph):
        raise ValueError(f'{what}: graph must be the (ptr, nbr, length) of mesh_edge_graph')
    ptr, nbr, length = graph
    if (ptr.dtype != torch.int32 or tuple(ptr.shape) != (V + 1,) or nbr.dtype != torch.int32 or nbr.dim() != 1
            or length.dtype != torch.float32 or length.shape != nbr.shape):
        raise ValueError(f'{what}: graph must hold ptr ({V + 1},) int32, nbr (E,) int32 and length (E,) float32 of this mesh')
    return tuple(t.detach().to(dev).contiguous() for t in graph)


def _edge_graph(p, f, dev, diagonals=False):
    """device tensors in, device tensors out"""
    V = int(p.shape[0])
    a = torch.cat((f[0], f[1], f[2], f[1], f[2], f[0]))
    b = torch.cat((f[1], f[2], f[0], f[0], f[1], f[2]))
    key = torch.unique(a * V + b)                   # sorted: by row, neighbours ascending, duplicates gone
    src, nbr = key // V, key % V
    keep = src != nbr                               # (a degenerate face names a vertex twice)
    src, nbr = src[keep].contiguous(), nbr[keep]
    ptr = torch.searchsorted(src, torch.arange(V + 1, device=dev)).to(torch.int32)
    src, nbr = src.to(torch.int32), nbr.to(torch.int32).contiguous()
    E = int(nbr.numel())
    length = torch.empty(E, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().fc_mesh_edge_lengths(_ptr(p), _ptr(src), _ptr(nbr), V, E, _ptr(length), _stream()), 'fc_mesh_edge_lengths')
    if diagonals:
        return _with_diagonals(p, f, dev, src, nbr, length)
    return ptr, nbr, length


def _with_diagonals(p, f, dev, src, nbr, length):
    """the sides' CSR slots (src, nbr int32, length) -> (ptr, nbr, length) of the sides and the unfolded diagonals
    (csrc/fc_mesh_graph.hip); sorting and compaction are torch, the geometry and the smallest-length rule are the kernels'"""
    V, F = int(p.shape[0]), int(f.shape[1])
    lib = _lib.load()
    # half-edge 3 f + k: corner k -> corner k + 1, opposite corner k + 2; a stable sort keeps equal keys in ascending face order
    a, b, o = f.t().reshape(-1), f[[1, 2, 0]].t().reshape(-1), f[[2, 0, 1]].t().reshape(-1)
    key = torch.minimum(a, b) * V + torch.maximum(a, b)
    key = torch.where((a == b) | (b == o) | (o == a), torch.full_like(key, V * V), key)          # (a degenerate face counts for no side)
    order = torch.sort(key, stable=True)
    N = 3 * F
    lo = torch.empty(N, dtype=torch.int32, device=dev)
    hi = torch.empty(N, dtype=torch.int32, device=dev)
    dlen = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.check(lib.fc_mesh_diagonals(_ptr(p), _ptr(f), V, F, _ptr(order.values.contiguous()), _ptr(order.indices.contiguous()), N, _ptr(lo),
                                     _ptr(hi), _ptr(dlen), _stream()), 'fc_mesh_diagonals')
    found = lo >= 0
    lo, hi, dlen = lo[found].to(torch.int64), hi[found].to(torch.int64), dlen[found]
    keys = torch.cat((src.to(torch.int64) * V + nbr.to(torch.int64), lo * V + hi, hi * V + lo))
    order = torch.sort(keys, stable=True)
    keys, lens = order.values.contiguous(), torch.cat((length, dlen, dlen))[order.indices].contiguous()
    N = int(keys.numel())
    head = torch.empty(N, dtype=torch.uint8, device=dev)
    msrc = torch.empty(N, dtype=torch.int32, device=dev)
    mnbr = torch.empty(N, dtype=torch.int32, device=dev)
    mlen = torch.empty(N, dtype=torch.float32, device=dev)
    _lib.check(lib.fc_mesh_graph_merge(_ptr(keys), _ptr(lens), N, V, _ptr(head), _ptr(msrc), _ptr(mnbr), _ptr(mlen), _stream()),
               'fc_mesh_graph_merge')
    head = head.to(torch.bool)
    msrc = msrc[head].to(torch.int64).contiguous()
    ptr = torch.searchsorted(msrc, torch.arange(V + 1, device=dev)).to(torch.int32)
    return ptr, mnbr[head].contiguous(), mlen[head].contiguous()


def _check_diagonals(graph, diagonals, what):
    if not isinstance(diagonals, bool):
        raise ValueError(f'{what}: diagonals must be True or False, got {diagonals!r}')
    if diagonals and graph is not None:
        raise ValueError(f'{what}: graph= already decides which edges there are: build it with mesh_edge_graph(pos, face, diagonals=True) '
                         'and leave diagonals at False')


def _mesh_on(pos, face, what):
    """a checked mesh -> (pos, face) on the device, face's vertex numbers checked (one synchronisation), and the device"""
    dev = _device_of(pos, 'geodesics')
    with _on(dev):
        return pos.detach().to(dev).contiguous(), _face_on(face, int(pos.shape[0]), dev, what), dev


def _prepare(pos, face, graph, what, diagonals=False):
    """-> (pos, face or None, graph) on the device, and the device; face is None where graph was given: nothing looked at it"""
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    if diagonals and 9 * face.shape[1] > 2 ** 31 - 1:
        raise ValueError(f'{what}: with diagonals a mesh has up to 9 directed edges per face, and edges are 32-bit indices in the kernels')
    if graph is None:
        p, f, dev = _mesh_on(pos, face, what)
        with _on(dev):
            return p, f, _edge_graph(p, f, dev, diagonals), dev
    dev = _device_of(pos, 'geodesics')
    with _on(dev):
        return pos.detach().to(dev).contiguous(), None, _graph_on(graph, int(pos.shape[0]), dev, what), dev


def _rows_per_call(rows_per_call, V, what):
    """the checked number of (V,) distance rows per launch; None: 256 MiB of them"""
    if rows_per_call is None:
        return max(1, _ROW_CHUNK_FLOATS // V)
    return _whole(rows_per_call, 1, 2 ** 63 - 1, what, 'rows_per_call', integral_floats=True)


def _batch_tables(pos_ptr, sample_ptr, V, S, what, name, sample_idx=None):
    """pos_ptr and the table `name` over the S samples: both None, or the (B+1,) range tables of a MeshBatch
    -> (B, max_range, host pos_ptr, host sample_ptr, on), on(device) being both tables on that device (None, None without tables).
    sample_idx: the samples of a mesh must be vertices of that mesh, checked on sample_idx's own device (one synchronisation)."""
    if (pos_ptr is None) != (sample_ptr is None):
        raise ValueError(f'{what}: pos_ptr and {name} go together (the ranges of a MeshBatch): give both or neither')
    if pos_ptr is None:
        return 1, V, None, None, lambda dev: (None, None)
    host_p, host_s = check_ptr(pos_ptr, V, what, 'pos_ptr'), check_ptr(sample_ptr, S, what, name)
    if len(host_p) != len(host_s):
        raise ValueError(f'{what}: pos_ptr describes {len(host_p) - 1} meshes, {name} {len(host_s) - 1}')
    B = len(host_p) - 1
    if sample_idx is not None:
        at = sample_idx.device
        mesh_of = torch.searchsorted(torch.tensor(host_p, dtype=torch.int64, device=at), sample_idx.contiguous(), right=True) - 1
        counts = torch.tensor([b - a for a, b in zip(host_s, host_s[1:])], dtype=torch.int64, device=at)
        if bool((mesh_of != torch.repeat_interleave(torch.arange(B, device=at), counts)).any()):
            raise ValueError(f'{what}: sample_idx of a mesh must name vertices of that mesh (rows of the union inside its pos_ptr range)')
    return (B, max(b - a for a, b in zip(host_p, host_p[1:])), host_p, host_s,
            lambda dev: (ptr_on(pos_ptr, host_p, dev), ptr_on(sample_ptr, host_s, dev)))


def _query_windows(S, slot_bytes):
    """the launches over S queries -> (queries per launch, its windows [(q0, nq), ...]): all at once where a query needs no
    workspace slot, else as many as keep the slots under 256 MiB"""
    per_call = max(1, min(S, _WORKSPACE_BYTES // slot_bytes)) if slot_bytes else S
    return per_call, [(q0, min(per_call, S - q0)) for q0 in range(0, S, per_call)]


def mesh_edge_graph(pos, face, diagonals=False):
    """(ptr (V+1,) int32, nbr (E,) int32, length (E,) float32): the undirected triangle sides, duplicates removed, as a CSR
    over the vertices with neighbours ascending (every side appears in both rows; a vertex in no face has an empty row), and
    length = sqrt((dx*dx + dy*dy) + dz*dz) in float32, every operation rounded on its own.  Pass it as `graph=` to the
    functions below to build it once per mesh.

    diagonals=True adds the UNFOLDED DIAGONALS (csrc/fc_mesh_graph.hip, restated in tests/_diagonal_graph_ref.py).  A path along
    triangle sides can only head in six directions, which keeps the side graph's distances 6 to 7 % above the true geodesic on
    average, up to 23 %, however fine the mesh; a diagonal joins the two vertices opposite an interior side across the unfolded
    pair of triangles, which about doubles the directions (1 to 1.5 % on average, up to 5 %, on the same meshes) and the
    degrees.  The result is a plain graph of the same layout, valid as `graph=` everywhere.
    Candidate side: {u, v}, u < v, contained in exactly two faces, counting only faces with three distinct vertices; c and d
    are the opposite vertices, c from the lower-numbered face, and must differ.  A boundary side (one face) and a non-manifold
    side (three or more) give nothing.  Unfolding, in float32, every operation rounded on its own:
        e = p_v - p_u, L2 = (ex*ex + ey*ey) + ez*ez (nothing when L2 == 0), L = sqrt(L2);
        for w in (c, d): r = p_w - p_u, x_w = ((rx*ex + ry*ey) + rz*ez) / L, y_w = sqrt(max(((rx*rx + ry*ry) + rz*rz) - x_w*x_w, 0));
        s = y_c + y_d (nothing when s <= 0); t = x_c + (x_d - x_c) * (y_c / s).
    The diagonal {c, d} exists when 0 < t < L, both strict: the straight segment from c to d crosses the shared side in the
    unfolded plane.  Its length is sqrt((x_c - x_d)*(x_c - x_d) + s*s).
    Merge: the union of sides and diagonals over undirected pairs; a pair that arises more than once (from two interior sides, or
    a diagonal that is also a side) keeps the smallest float32 length.  Every pair is computed once, in the orientation above,
    so both CSR rows hold the same bits.  Diagonals come from faces, so in the union of a MeshBatch none crosses meshes."""
    p, _, graph, _ = _prepare(pos, face, None, 'mesh_edge_graph', diagonals)
    return tuple(t.to(pos.device) for t in graph)


def geodesic_distances(pos, face, sources, graph=None, rows_per_call=None, return_sweeps=False, diagonals=False):
    """(S,V) float32: row k holds the edge-graph distance from vertex sources[k] to every vertex, +inf where there is no
    path.  d is the least fixpoint of d[source] = 0, d[v] = min_u fl32(d[u] + length(u,v)): the bits of a heap Dijkstra
    with float32 additions.  One workgroup per row, launched rows_per_call rows at a time (default: 256 MiB of rows), so
    for host tensors the device never holds more than one chunk.  return_sweeps: also the (S,) int32 sweep counts.
    diagonals (here and in every function below that builds the graph itself when graph is None): over
    mesh_edge_graph(pos, face, diagonals=True), the sides and the unfolded diagonals; together with an explicit graph= it raises
    ValueError, because the graph already decides."""
    what = 'geodesic_distances'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sources, V, what, 'sources')
    S = int(sources.numel())
    rows_per_call = min(_rows_per_call(rows_per_call, V, what), S)
    p, _, (ptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    E = int(nbr.numel())
    out = torch.empty((S, V), dtype=torch.float32, device=pos.device)
    with _on(dev):
        src = sources.detach().to(dev).contiguous()
        sweeps = torch.empty((S, 2), dtype=torch.int32, device=dev)
        for s0 in range(0, S, rows_per_call):
            s1 = min(S, s0 + rows_per_call)
            rows = out[s0:s1] if out.device == dev else torch.empty((s1 - s0, V), dtype=torch.float32, device=dev)
            _lib.check(lib.fc_geodesic_rows(_ptr(ptr), _ptr(nbr), _ptr(length), V, E, _ptr(src[s0:s1]), s1 - s0, _ptr(rows),
                                            _ptr(sweeps[s0:s1]), _stream()), 'fc_geodesic_rows')
            if rows.device != out.device:
                out[s0:s1] = rows.to(out.device)
    return (out, sweeps[:, 0].to(pos.device)) if return_sweeps else out


def nearest_sample(pos, face, sample_idx, pos_ptr=None, sample_ptr=None, graph=None, return_sweeps=False, diagonals=False):
    """(label (V,) int64, dist (V,) float32): for every vertex the edge-graph distance to the nearest of the vertices
    sample_idx (S,) int64, and which one: label is a POSITION in sample_idx.  Labels are taken after the distances have
    converged, over the tight edges fl32(d[u] + length) == d[v]: label[v] is the smallest position whose sample reaches v
    along tight edges, so exact ties go to the lower position, a vertex listed twice counts at its lower position, and the
    result does not depend on any schedule.  A vertex no sample reaches has dist +inf and label -1.
    pos_ptr, sample_ptr: both None, or the (B+1,) int64 range tables of a MeshBatch (batch.pos_ptr over the rows of pos,
    batch.ptr over sample_idx, whose entries are rows of the union's pos): every mesh searches its own samples only, one
    workgroup per mesh in one launch; a label is the position inside the mesh's own sample range plus that range's start.
    return_sweeps: also the (B,2) int32 sweep counts (distance loop, label loop) per mesh."""
    what = 'nearest_sample'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    S = int(sample_idx.numel())
    B, max_range, _, host_s, tables_on = _batch_tables(pos_ptr, sample_ptr, V, S, what, 'sample_ptr', sample_idx)
    if host_s is not None and any(b == a for a, b in zip(host_s, host_s[1:])):
        raise ValueError(f'{what}: a mesh of the batch has no samples')
    p, _, (ptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    E = int(nbr.numel())
    with _on(dev):
        src = sample_idx.detach().to(dev).contiguous()
        pp, sp = tables_on(dev)
        nbytes = lib.fc_geodesic_workspace_bytes(V, max_range)
        ws = _scratch(nbytes, dev, None)
        dist = torch.empty(V, dtype=torch.float32, device=dev)
        label = torch.empty(V, dtype=torch.int64, device=dev)
        sweeps = torch.empty((B, 2), dtype=torch.int32, device=dev)
        _lib.check(lib.fc_geodesic_nearest(_ptr(ptr), _ptr(nbr), _ptr(length), V, E, _ptr(pp), _ptr(src), _ptr(sp), S, B, max_range,
                                           _ptr(dist), _ptr(label), _ptr(sweeps), _ptr(ws), nbytes, _stream()), 'fc_geodesic_nearest')
    out = (label.to(pos.device), dist.to(pos.device))
    return out + (sweeps.to(pos.device),) if return_sweeps else out


def samples_to_nearest(pos, face, samples, diagonals=False):
    """(V,) int64: for every vertex the position in `samples` of its nearest sample (fcutils' samplesToNearest and its
    argument order; by the edge-graph metric, ties to the lower position, -1 where no sample is reachable)."""
    return nearest_sample(pos, face, samples, diagonals=diagonals)[0]


def compose_map(labels_tem2tar, labels_tem2sour, pos, face, diagonals=False):
    """(V,) int64 labels of the source mesh's vertices on the target (fcutils' composeMap and its argument order): template
    vertex l corresponds to vertex labels_tem2sour[l] - 1 of the source mesh (pos, face; 1-BASED, as in the label files)
    and to labels_tem2tar[l] on the target, so source vertex labels_tem2sour[l] - 1 gets labels_tem2tar[l] (the last l wins
    where a vertex is hit twice), and every vertex that was not hit copies the label of the nearest vertex that was (-1
    where none is reachable).  labels_tem2tar is passed through as it is."""
    what = 'compose_map'
    _check_mesh(pos, face, what)
    V = int(pos.shape[0])
    if not torch.is_tensor(labels_tem2tar) or labels_tem2tar.dim() != 1 or labels_tem2tar.dtype != torch.int64:
        raise ValueError(f'{what}: labels_tem2tar must be a 1-D int64 tensor')
    if not torch.is_tensor(labels_tem2sour) or labels_tem2sour.shape != labels_tem2tar.shape or labels_tem2sour.dtype != torch.int64:
        raise ValueError(f'{what}: labels_tem2sour must be an int64 tensor of labels_tem2tar\'s shape')
    hit_by = _check_index(labels_tem2sour - 1, V, what, 'labels_tem2sour - 1').to(pos.device)
    tar = labels_tem2tar.to(pos.device)
    last = torch.full((V,), -1, dtype=torch.int64, device=pos.device)
    last.scatter_reduce_(0, hit_by, torch.arange(hit_by.numel(), device=pos.device), 'amax')
    hit = torch.nonzero(last >= 0)[:, 0]            # the vertices that were hit, ascending: the sources
    label, _ = nearest_sample(pos, face, hit, diagonals=diagonals)
    via = hit[label.clamp(min=0)]                   # (a vertex that was hit is its own nearest: distance 0, lowest position)
    return torch.where(label >= 0, tar[last[via]], torch.full_like(label, -1))


def _face_areas(p, f, dev):
    V, F = int(p.shape[0]), int(f.shape[1])
    area = torch.empty(F, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().fc_face_areas(_ptr(p), _ptr(f), V, F, _ptr(area), _stream()), 'fc_face_areas')
    return area


def _segment_sum(values, keys, K, divisor, dev):
    """out[k] = (the values whose key is k, added in float32 in their order of appearance) / divisor, for k in [0,K): a stable
    sort by key and one thread per range; keys below 0 contribute to nothing"""
    order = torch.sort(keys, stable=True)
    ptr = torch.searchsorted(order.values.contiguous(), torch.arange(K + 1, device=dev))
    x = values[order.indices].contiguous()
    out = torch.empty(K, dtype=torch.float32, device=dev)
    _lib.check(_lib.load().fc_segment_sum_f32(_ptr(x), _ptr(ptr), int(x.numel()), K, float(divisor), _ptr(out), _stream()),
               'fc_segment_sum_f32')
    return out


def vertex_masses(pos, face):
    """(V,) float32 lumped vertex masses: one third of the sum of the incident triangle areas, the areas added in float32 in
    the order (corner 0 of every face, corner 1, corner 2; faces ascending) -- a fixed order, the same bits on every run."""
    what = 'vertex_masses'
    _check_mesh(pos, face, what)
    p, f, dev = _mesh_on(pos, face, what)
    with _on(dev):
        return _segment_sum(_face_areas(p, f, dev).repeat(3), f.reshape(-1), int(p.shape[0]), 3.0, dev).to(pos.device)


def sample_weights(pos, face, sample_idx, pos_ptr=None, sample_ptr=None, graph=None, diagonals=False):
    """(S,1) float32, the reference's data.w (fcutils.weights): the lumped vertex masses (vertex_masses) summed onto each
    vertex's nearest sample (nearest_sample; with the two ptr tables per mesh of a MeshBatch).  The sum of a sample runs in
    float32 over its vertices in ascending order: no float atomics, two runs give the same bits.  A vertex no sample reaches
    (label -1) contributes to nothing."""
    what = 'sample_weights'
    label, _ = nearest_sample(pos, face, sample_idx, pos_ptr, sample_ptr, graph, diagonals=diagonals)
    dev = _device_of(pos, 'geodesics')
    with _on(dev):
        mass = vertex_masses(pos, face).to(dev)
        w = _segment_sum(mass, label.to(dev), int(sample_idx.numel()), 1.0, dev)
    return w[:, None].to(pos.device)


def surface_area(pos, face):
    """The mesh's area as a Python float: the float32 triangle areas added in float64."""
    what = 'surface_area'
    _check_mesh(pos, face, what)
    p, f, dev = _mesh_on(pos, face, what)
    with _on(dev):
        return float(_face_areas(p, f, dev).to(torch.float64).sum())


def geodesic_error(pos, face, pred, target, normalize=True, graph=None, rows_per_call=None, diagonals=False):
    """(M,) float32: the edge-graph distance on the template (pos, face) between the predicted vertex pred[m] and the true
    vertex target[m] (both (M,) int64; e.g. LinearCrossEntropy.predict(h)[0][:, 0] and the labels), divided by sqrt(area)
    when normalize (the usual correspondence-benchmark convention).  Distance rows are solved for the DISTINCT targets only,
    rows_per_call at a time (geodesic_distances): the V x V matrix is never built."""
    what = 'geodesic_error'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(target, V, what, 'target')
    _check_index(pred, V, what, 'pred')
    if pred.shape != target.shape:
        raise ValueError(f'{what}: pred {tuple(pred.shape)} and target {tuple(target.shape)} must have the same length')
    if pred.device != target.device:
        raise ValueError(f'{what}: pred is on {pred.device}, target on {target.device}')
    dev = _device_of(pos, 'geodesics')
    with _on(dev):
        if graph is None:
            graph = _prepare(pos, face, None, what, diagonals)[2]
        uniq, inv = torch.unique(target.to(dev), return_inverse=True)
        pr = pred.to(dev)
        U = int(uniq.numel())
        step = _rows_per_call(rows_per_call, V, what)
        p = pos.detach().to(dev)
        err = torch.empty(int(pr.numel()), dtype=torch.float32, device=dev)
        for u0 in range(0, U, step):
            u1 = min(U, u0 + step)
            rows = geodesic_distances(p, face, uniq[u0:u1], graph=graph)
            mine = torch.nonzero((inv >= u0) & (inv < u1))[:, 0]
            err[mine] = rows[inv[mine] - u0, pr[mine]]
        if normalize:
            err = err / torch.full_like(err, surface_area(pos, face) ** 0.5)
    return err.to(pos.device)


def correspondence_curve(err, thresholds):
    """(T,) float64: the fraction of the entries of err that are <= thresholds[j] (the cumulative geodesic-error curve).
    Plain torch on err's device; NaN and +inf errors count as misses."""
    if not torch.is_tensor(err) or err.dim() != 1 or not err.is_floating_point() or err.numel() < 1:
        raise ValueError('correspondence_curve: err must be a non-empty 1-D floating-point tensor')
    t = torch.as_tensor(thresholds, dtype=err.dtype, device=err.device).reshape(-1)
    hits = (err[None, :] <= t[:, None]).sum(1).to(torch.float64)
    return hits / torch.full_like(hits, err.numel())          # (by a tensor: one rounded division)
