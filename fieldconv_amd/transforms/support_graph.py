"""Support graph of a point set (the data contract of the reference's SupportGraph transform): farthest-point sampling,
then every sample's neighbours within epsilon.  The arithmetic runs on the ROCm device (csrc/fc_support.hip) whatever
device the input is on; results go back to the input's device, so the transform also serves as a CPU-side
`pre_transform`.  There is no CPU arithmetic path."""
import math

import torch

from .._launch import device_of as _device_of, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from ..pooling import check_ptr, per_mesh, ptr_on


def _check_pos(pos, what):
    if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[1] != 3:
        raise ValueError(f'{what}: pos must be an (N,3) tensor, got {tuple(pos.shape) if torch.is_tensor(pos) else type(pos).__name__}')
    if pos.shape[0] < 1:
        raise ValueError(f'{what}: pos holds no points')
    if pos.shape[0] > 2 ** 31 - 1:
        raise ValueError(f'{what}: at most 2^31 - 1 points')
    if not pos.is_floating_point():
        raise ValueError(f'{what}: pos must be a floating-point tensor, got {pos.dtype}')


def _check_epsilon(epsilon, what):
    try:
        eps = float(epsilon)
    except (TypeError, ValueError):
        raise ValueError(f'{what}: epsilon must be a number, got {epsilon!r}') from None
    if not (eps > 0 and math.isfinite(eps)) or not (float(torch.tensor(eps, dtype=torch.float32)) > 0):
        raise ValueError(f'{what}: epsilon must be positive and finite (in float32), got {epsilon!r}')
    return eps


def _check_k(max_num_neighbors, what):
    return _whole(max_num_neighbors, 1, 2 ** 63 - 1, what, 'max_num_neighbors', integral_floats=True)


def _on_device(pos):
    """pos as contiguous float32 on the ROCm device it is on (CPU input: the current device)."""
    dev = _device_of(pos, 'support graphs')
    return pos.detach().to(device=dev, dtype=torch.float32).contiguous(), dev


def farthest_point_sample(pos, n_samples, start=0):
    """(n_samples,) int64 indices into pos in selection order, idx[0] = start: each next sample is the point farthest (in
    squared fp32 distance) from those already taken, ties to the lowest index; no point is taken twice, even where
    positions repeat.  pos: (N,3); 1 <= n_samples <= N; 0 <= start < N."""
    _check_pos(pos, 'farthest_point_sample')
    N = int(pos.shape[0])
    S = _whole(n_samples, 1, N, 'farthest_point_sample', 'n_samples', integral_floats=True)
    start = _whole(start, 0, N - 1, 'farthest_point_sample', 'start', integral_floats=True)
    from .. import _lib
    lib = _lib.load()
    p, dev = _on_device(pos)
    with _on(dev):
        st = _stream()
        nbytes = lib.fc_fps_workspace_bytes(N)
        ws = _scratch(nbytes, dev)
        idx = torch.empty(S, dtype=torch.int64, device=dev)
        _lib.check(lib.fc_fps(_ptr(p), N, S, start, _ptr(idx), _ptr(ws), nbytes, st), 'fc_fps')
    return idx.to(pos.device)


def radius_edges(pos, epsilon, max_num_neighbors=512):
    """(E,2) int64 rows [query, neighbour] for every pair with squared fp32 distance < fp32(epsilon)^2 (each point is its own
    neighbour), grouped by query in ascending order, each query's neighbours ascending.  A query with more than
    max_num_neighbors such points keeps the max_num_neighbors nearest, ties to the lower index."""
    _check_pos(pos, 'radius_edges')
    eps = _check_epsilon(epsilon, 'radius_edges')
    K = _check_k(max_num_neighbors, 'radius_edges')
    from .. import _lib
    lib = _lib.load()
    p, dev = _on_device(pos)
    N = int(pos.shape[0])
    with _on(dev):
        st = _stream()
        nbytes = lib.fc_radius_workspace_bytes(N)
        ws = _scratch(nbytes, dev)
        _lib.check(lib.fc_radius_count(_ptr(p), N, eps, K, _ptr(ws), nbytes, st), 'fc_radius_count')
        off = lib.fc_radius_edge_count_ptr(_ptr(ws), N) - ws.data_ptr()
        E = int(ws[off:off + 8].view(torch.int64).item())          # the one synchronisation: E sizes the output
        edges = torch.empty((E, 2), dtype=torch.int64, device=dev)
        _lib.check(lib.fc_radius_fill(_ptr(p), N, eps, K, E, _ptr(edges), _ptr(ws), nbytes, st), 'fc_radius_fill')
    return edges.to(pos.device)


def farthest_point_sample_batched(pos, pos_ptr, n_samples, start=0):
    """farthest_point_sample for B point sets at once, one workgroup per set: set b is pos[pos_ptr[b]:pos_ptr[b+1]] (pos_ptr:
    (B+1,) int64, on the host or on the device; its values are checked on the host, see fieldconv_amd.pooling), n_samples and
    start one integer for all sets or one per set, 1 <= n_samples[b] <= n_b, 0 <= start[b] < n_b.  Returns the (sum n_samples,)
    int64 indices, set after set in selection order, each LOCAL to its set (add pos_ptr[b] for rows of pos): index for index what
    farthest_point_sample gives for the set alone."""
    what = 'farthest_point_sample_batched'
    _check_pos(pos, what)
    N = int(pos.shape[0])
    host = check_ptr(pos_ptr, N, what, 'pos_ptr')
    B = len(host) - 1
    S, st = per_mesh(n_samples, B, what, 'n_samples'), per_mesh(start, B, what, 'start')
    for b in range(B):
        n_b = host[b + 1] - host[b]
        S[b] = _whole(S[b], 1, n_b, what, 'n_samples', f' of mesh {b}', integral_floats=True)
        st[b] = _whole(st[b], 0, n_b - 1, what, 'start', f' of mesh {b}', integral_floats=True)
    from .. import _lib
    lib = _lib.load()
    p, dev = _on_device(pos)
    out_ptr = [0]
    for v in S:
        out_ptr.append(out_ptr[-1] + v)
    with _on(dev):
        stream = _stream()
        tables = torch.tensor([S, st, out_ptr[:-1]], dtype=torch.int64).to(dev)
        ptr_d = ptr_on(pos_ptr, host, dev)
        nbytes = lib.fc_fps_batched_workspace_bytes(N)
        ws = _scratch(nbytes, dev)
        idx = torch.empty(out_ptr[-1], dtype=torch.int64, device=dev)
        _lib.check(lib.fc_fps_batched(_ptr(p), _ptr(ptr_d), N, B, _ptr(tables[0]), _ptr(tables[1]), _ptr(tables[2]), out_ptr[-1], _ptr(idx),
                                      _ptr(ws), nbytes, stream), 'fc_fps_batched')
    return idx.to(pos.device)


def radius_edges_batched(pos, ptr, epsilon, max_num_neighbors=512):
    """radius_edges for B point sets at once: set b is pos[ptr[b]:ptr[b+1]] (ptr: (B+1,) int64, host or device, checked on the
    host) and a point's neighbours are searched inside its own set only.  (E,2) int64 rows [query, neighbour] numbered in the
    union, queries ascending, neighbours ascending: the rows radius_edges gives for each set alone plus ptr[b], set after set.
    One epsilon and one max_num_neighbors for the batch; one synchronisation (the edge count), as in radius_edges."""
    what = 'radius_edges_batched'
    _check_pos(pos, what)
    eps = _check_epsilon(epsilon, what)
    K = _check_k(max_num_neighbors, what)
    N = int(pos.shape[0])
    host = check_ptr(ptr, N, what)
    B = len(host) - 1
    if N + 256 * B >= 2 ** 31 - 1:
        raise ValueError(f'{what}: points + 256 * meshes must stay below 2^31')
    from .. import _lib
    lib = _lib.load()
    p, dev = _on_device(pos)
    with _on(dev):
        st = _stream()
        ptr_d = ptr_on(ptr, host, dev)
        nbytes = lib.fc_radius_workspace_bytes(N)
        ws = _scratch(nbytes, dev)
        _lib.check(lib.fc_radius_count_batched(_ptr(p), _ptr(ptr_d), N, B, eps, K, _ptr(ws), nbytes, st), 'fc_radius_count_batched')
        off = lib.fc_radius_edge_count_ptr(_ptr(ws), N) - ws.data_ptr()
        E = int(ws[off:off + 8].view(torch.int64).item())          # the one synchronisation: E sizes the output
        edges = torch.empty((E, 2), dtype=torch.int64, device=dev)
        _lib.check(lib.fc_radius_fill_batched(_ptr(p), _ptr(ptr_d), N, B, eps, K, E, _ptr(edges), _ptr(ws), nbytes, st),
                   'fc_radius_fill_batched')
    return edges.to(pos.device)


class SupportGraph(object):
    """Filter-support edges of a mesh's vertices (the reference's transforms.SupportGraph contract; not the convolution's
    internal fieldconv_amd.graph.SupportGraph).

    data.sample_idx, when present, selects the points; otherwise, with sample_n set and sample_n <= N, farthest-point
    sampling takes exactly sample_n points (from a start drawn with torch.randint(N, (1,), generator=generator), or 0 when
    random_start is False), sorted ascending; otherwise every point.  The selection is stored as data.sample_idx and
    data.supp_edges = radius_edges(pos[sample_idx], epsilon, max_num_neighbors), numbered within the sample.

    A fieldconv_amd.data.MeshBatch that has pos / pos_ptr goes through the batched kernels, all meshes in one pass each:
    every mesh gets min(sample_n, n_b) samples (one random start per mesh, drawn in mesh order), the batch gets sample_idx
    (rows of the union's pos, ascending), ptr, batch, supp_edges (numbered in the union's sample, neighbours from the query's
    own mesh only) and edge_ptr -- mesh for mesh what the single-mesh call gives.  A batch that already has sample_idx keeps it
    (and its ptr)."""

    def __init__(self, epsilon, sample_n=None, max_num_neighbors=512, random_start=True, generator=None):
        self.epsilon = _check_epsilon(epsilon, 'SupportGraph')
        if sample_n is not None and (isinstance(sample_n, bool) or int(sample_n) != sample_n or sample_n < 1):
            raise ValueError(f'SupportGraph: sample_n must be None or an integer >= 1, got {sample_n!r}')
        self.sample_n = None if sample_n is None else int(sample_n)
        self.max_num_neighbors = _check_k(max_num_neighbors, 'SupportGraph')
        self.random_start = random_start
        self.generator = generator

    def _call_batch(self, data):
        pos = data.pos
        _check_pos(pos, 'SupportGraph')
        pp = check_ptr(data.pos_ptr, int(pos.shape[0]), 'SupportGraph', 'pos_ptr')
        B = len(pp) - 1
        n_full = [pp[b + 1] - pp[b] for b in range(B)]
        if getattr(data, 'sample_idx', None) is None:
            if min(n_full) < 1:
                raise ValueError('SupportGraph: a mesh of the batch holds no points')
            if self.sample_n is not None:
                S = [min(self.sample_n, n) for n in n_full]
                starts = [int(torch.randint(n, (1,), generator=self.generator)) if self.random_start else 0 for n in n_full]
                local = farthest_point_sample_batched(pos, data.pos_ptr, S, starts)
                first = torch.repeat_interleave(torch.tensor(pp[:-1], dtype=torch.int64), torch.tensor(S, dtype=torch.int64))
                # the meshes' row ranges ascend with the mesh, so one sort orders every mesh's samples and keeps the meshes apart
                data.sample_idx = (local + first.to(local.device)).sort()[0]
            else:
                S = n_full
                data.sample_idx = torch.arange(int(pos.shape[0]), device=pos.device)
            data._set_ranges(S, pos.device)
        elif getattr(data, 'ptr', None) is None:
            raise ValueError('SupportGraph: a batch with sample_idx needs ptr, the ranges of the sampled vertices')
        sample_idx = data.sample_idx
        check_ptr(data.ptr, int(sample_idx.shape[0]), 'SupportGraph')
        data.supp_edges = radius_edges_batched(pos[sample_idx.to(pos.device)], data.ptr, self.epsilon, self.max_num_neighbors)
        # queries ascend, so mesh b's rows are those between the first query >= ptr[b] and the first >= ptr[b+1]
        data.edge_ptr = torch.searchsorted(data.supp_edges[:, 0].contiguous(), data.ptr.to(data.supp_edges.device))
        return data

    def __call__(self, data):
        if getattr(data, 'pos_ptr', None) is not None:
            return self._call_batch(data)
        pos = data.pos
        _check_pos(pos, 'SupportGraph')
        N = int(pos.shape[0])
        sample_idx = getattr(data, 'sample_idx', None)
        if sample_idx is None:
            if self.sample_n is not None and self.sample_n <= N:
                start = int(torch.randint(N, (1,), generator=self.generator)) if self.random_start else 0
                sample_idx = farthest_point_sample(pos, self.sample_n, start).sort()[0]
            else:
                sample_idx = torch.arange(N, device=pos.device)
            data.sample_idx = sample_idx
        data.supp_edges = radius_edges(pos[sample_idx.to(pos.device)], self.epsilon, self.max_num_neighbors)
        return data

    def __repr__(self):
        return '{}(epsilon={}, sample_n={}, max_num_neighbors={})'.format(self.__class__.__name__, self.epsilon, self.sample_n,
                                                                         self.max_num_neighbors)
