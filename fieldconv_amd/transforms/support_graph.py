"""Support graph of a point set (the data contract of the reference's SupportGraph transform): farthest-point sampling,
then every sample's neighbours within epsilon.  The arithmetic runs on the ROCm device (csrc/fc_support.hip) whatever
device the input is on; results go back to the input's device, so the transform also serves as a CPU-side
`pre_transform`.  There is no CPU arithmetic path."""
import ctypes
import math

import torch


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
    if isinstance(max_num_neighbors, bool) or int(max_num_neighbors) != max_num_neighbors or max_num_neighbors < 1:
        raise ValueError(f'{what}: max_num_neighbors must be an integer >= 1, got {max_num_neighbors!r}')
    return int(max_num_neighbors)


def _on_device(pos):
    """pos as contiguous float32 on the ROCm device it is on (CPU input: the current device)."""
    if pos.is_cuda:
        dev = pos.device
    else:
        if not torch.cuda.is_available():
            raise RuntimeError('fieldconv_amd support graphs are computed on a ROCm device and none is visible; there is no CPU path')
        dev = torch.device('cuda', torch.cuda.current_device())
    return pos.detach().to(device=dev, dtype=torch.float32).contiguous(), dev


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def farthest_point_sample(pos, n_samples, start=0):
    """(n_samples,) int64 indices into pos in selection order, idx[0] = start: each next sample is the point farthest (in
    squared fp32 distance) from those already taken, ties to the lowest index; no point is taken twice, even where
    positions repeat.  pos: (N,3); 1 <= n_samples <= N; 0 <= start < N."""
    _check_pos(pos, 'farthest_point_sample')
    N = int(pos.shape[0])
    if isinstance(n_samples, bool) or int(n_samples) != n_samples or not 1 <= n_samples <= N:
        raise ValueError(f'farthest_point_sample: n_samples must be an integer in [1, {N}], got {n_samples!r}')
    if isinstance(start, bool) or int(start) != start or not 0 <= start < N:
        raise ValueError(f'farthest_point_sample: start must be an integer in [0, {N}), got {start!r}')
    from .. import _lib
    lib = _lib.load()
    p, dev = _on_device(pos)
    S = int(n_samples)
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nbytes = lib.fc_fps_workspace_bytes(N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        idx = torch.empty(S, dtype=torch.int64, device=dev)
        _lib.check(lib.fc_fps(_ptr(p), N, S, int(start), _ptr(idx), _ptr(ws), nbytes, st), 'fc_fps')
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
    with torch.cuda.device(dev):
        st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        nbytes = lib.fc_radius_workspace_bytes(N)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.fc_radius_count(_ptr(p), N, eps, K, _ptr(ws), nbytes, st), 'fc_radius_count')
        off = lib.fc_radius_edge_count_ptr(_ptr(ws), N) - ws.data_ptr()
        E = int(ws[off:off + 8].view(torch.int64).item())          # the one synchronisation: E sizes the output
        edges = torch.empty((E, 2), dtype=torch.int64, device=dev)
        _lib.check(lib.fc_radius_fill(_ptr(p), N, eps, K, E, _ptr(edges), _ptr(ws), nbytes, st), 'fc_radius_fill')
    return edges.to(pos.device)


class SupportGraph(object):
    """Filter-support edges of a mesh's vertices (the reference's transforms.SupportGraph contract; not the convolution's
    internal fieldconv_amd.graph.SupportGraph).

    data.sample_idx, when present, selects the points; otherwise, with sample_n set and sample_n <= N, farthest-point
    sampling takes exactly sample_n points (from a start drawn with torch.randint(N, (1,), generator=generator), or 0 when
    random_start is False), sorted ascending; otherwise every point.  The selection is stored as data.sample_idx and
    data.supp_edges = radius_edges(pos[sample_idx], epsilon, max_num_neighbors), numbered within the sample."""

    def __init__(self, epsilon, sample_n=None, max_num_neighbors=512, random_start=True, generator=None):
        self.epsilon = _check_epsilon(epsilon, 'SupportGraph')
        if sample_n is not None and (isinstance(sample_n, bool) or int(sample_n) != sample_n or sample_n < 1):
            raise ValueError(f'SupportGraph: sample_n must be None or an integer >= 1, got {sample_n!r}')
        self.sample_n = None if sample_n is None else int(sample_n)
        self.max_num_neighbors = _check_k(max_num_neighbors, 'SupportGraph')
        self.random_start = random_start
        self.generator = generator

    def __call__(self, data):
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
