"""SupportGraph by the mesh's own metric: geodesic farthest-point sampling, then every sample's neighbours inside a geodesic
ball (fieldconv_amd.geodesic_sampling, csrc/fc_geodesic_fps.hip) in place of the Euclidean fc_fps / fc_radius_*.  Two parts of
a surface that pass close to each other in space -- a hand near a thigh, finger against finger -- are neither under-sampled nor
joined: distances run along the triangle sides.  The arithmetic runs on the ROCm device whatever device the input is on;
results go back to data.pos's device.  There is no CPU arithmetic path."""
import torch

from ..geodesic import mesh_edge_graph
from ..geodesic_sampling import (geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched, geodesic_radius_edges)
from .support_graph import _check_epsilon, _check_k


class GeodesicSupportGraph(object):
    """transforms.SupportGraph's contract, field for field, by the edge-graph metric; needs data.face (3,F) int64 beside
    data.pos (V,3) float32.

    data.sample_idx, when present, selects the vertices (it must be ascending); otherwise, with sample_n set and sample_n <= V,
    geodesic farthest-point sampling takes exactly sample_n vertices (from a start drawn with torch.randint(V, (1,),
    generator=generator), or 0 when random_start is False), sorted ascending; otherwise every vertex.  Vertices in no face and
    further components are sampled first (their distance is +inf).  The selection is stored as data.sample_idx and
    data.supp_edges = geodesic_radius_edges(pos, face, sample_idx, epsilon, max_num_neighbors), numbered within the sample.

    A fieldconv_amd.data.MeshBatch goes through the batched launches, one workgroup per mesh or query: every mesh gets
    min(sample_n, n_b) samples (one random start per mesh, drawn in mesh order), the batch gets sample_idx (rows of the union's
    pos, ascending), ptr, batch, supp_edges (numbered in the union's sample, neighbours from the query's own mesh only) and
    edge_ptr -- mesh for mesh what the single-mesh call gives.  A batch that already has sample_idx keeps it (and its ptr).
    SampleWeights and FCPrecomp consume the result unchanged.

    diagonals=True measures over mesh_edge_graph(pos, face, diagonals=True), the sides and the unfolded diagonals: distances
    about 1 % above the true geodesic instead of 6 %, so epsilon cuts a rounder ball.  Use the same setting in ComputeLogXPort."""

    def __init__(self, epsilon, sample_n=None, max_num_neighbors=512, random_start=True, generator=None, diagonals=False):
        self.epsilon = _check_epsilon(epsilon, 'GeodesicSupportGraph')
        if sample_n is not None and (isinstance(sample_n, bool) or int(sample_n) != sample_n or sample_n < 1):
            raise ValueError(f'GeodesicSupportGraph: sample_n must be None or an integer >= 1, got {sample_n!r}')
        self.sample_n = None if sample_n is None else int(sample_n)
        self.max_num_neighbors = _check_k(max_num_neighbors, 'GeodesicSupportGraph')
        self.random_start = random_start
        self.generator = generator
        if not isinstance(diagonals, bool):
            raise ValueError(f'GeodesicSupportGraph: diagonals must be True or False, got {diagonals!r}')
        self.diagonals = diagonals

    def _start(self, n):
        return int(torch.randint(n, (1,), generator=self.generator)) if self.random_start else 0

    def _call_batch(self, data, graph):
        from ..pooling import check_ptr
        pos = data.pos
        pp = check_ptr(data.pos_ptr, int(pos.shape[0]), 'GeodesicSupportGraph', 'pos_ptr')
        B = len(pp) - 1
        n_full = [pp[b + 1] - pp[b] for b in range(B)]
        if getattr(data, 'sample_idx', None) is None:
            if min(n_full) < 1:
                raise ValueError('GeodesicSupportGraph: a mesh of the batch holds no vertices')
            if self.sample_n is not None:
                S = [min(self.sample_n, n) for n in n_full]
                starts = [self._start(n) for n in n_full]
                local = geodesic_farthest_point_sample_batched(pos, data.face, data.pos_ptr, S, starts, graph=graph)
                first = torch.repeat_interleave(torch.tensor(pp[:-1], dtype=torch.int64), torch.tensor(S, dtype=torch.int64))
                # the meshes' row ranges ascend with the mesh, so one sort orders every mesh's samples and keeps the meshes apart
                data.sample_idx = (local + first.to(local.device)).sort()[0]
            else:
                S = n_full
                data.sample_idx = torch.arange(int(pos.shape[0]), device=pos.device)
            data._set_ranges(S, pos.device)
        elif getattr(data, 'ptr', None) is None:
            raise ValueError('GeodesicSupportGraph: a batch with sample_idx needs ptr, the ranges of the sampled vertices')
        data.supp_edges = geodesic_radius_edges(pos, data.face, data.sample_idx.to(pos.device), self.epsilon, self.max_num_neighbors,
                                                pos_ptr=data.pos_ptr, sample_ptr=data.ptr, graph=graph)
        # queries ascend, so mesh b's rows are those between the first query >= ptr[b] and the first >= ptr[b+1]
        data.edge_ptr = torch.searchsorted(data.supp_edges[:, 0].contiguous(), data.ptr.to(data.supp_edges.device))
        return data

    def __call__(self, data):
        if getattr(data, 'face', None) is None:
            raise ValueError('GeodesicSupportGraph: data needs face (3,F) beside pos: the metric is the mesh\'s')
        graph = mesh_edge_graph(data.pos, data.face, self.diagonals)          # built once, shared by the sampler and the ball search
        if getattr(data, 'pos_ptr', None) is not None:
            return self._call_batch(data, graph)
        pos = data.pos
        V = int(pos.shape[0])
        sample_idx = getattr(data, 'sample_idx', None)
        if sample_idx is None:
            if self.sample_n is not None and self.sample_n <= V:
                sample_idx = geodesic_farthest_point_sample(pos, data.face, self.sample_n, self._start(V), graph=graph).sort()[0]
            else:
                sample_idx = torch.arange(V, device=pos.device)
            data.sample_idx = sample_idx
        data.supp_edges = geodesic_radius_edges(pos, data.face, sample_idx.to(pos.device), self.epsilon, self.max_num_neighbors, graph=graph)
        return data

    def __repr__(self):
        return '{}(epsilon={}, sample_n={}, max_num_neighbors={}{})'.format(self.__class__.__name__, self.epsilon, self.sample_n,
                                                                           self.max_num_neighbors, ', diagonals=True' if self.diagonals else '')
