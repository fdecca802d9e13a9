"""A coarser sample level of a mesh and the two transfers that join it to the fine one: what an encoder / decoder needs to
change resolution inside a network.  Built on the ROCm device from the package's own pieces (farthest-point sampling,
GeodesicSupportGraph, ComputeLogXPort, fieldconv_amd.transfer.level_transfer); results stay on data.pos's device, the two plans
on the ROCm device."""
import torch

from ..data.synthetic import SupportData
from ..transfer import _check_coarse, _check_knn, interpolation_plan, level_transfer
from .compute_log_xport import ComputeLogXPort
from ..geodesic_sampling import geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched
from .geodesic_support_graph import GeodesicSupportGraph
from .support_graph import _check_epsilon, _check_k, farthest_point_sample, farthest_point_sample_batched


class CoarsenSamples(object):
    """Applied to a fine-level data (pos, face, sample_idx ascending, w -- after GeodesicSupportGraph and ComputeLogXPort) it
    returns a NEW coarse-level data object that shares pos and face and carries

        coarse          (S_c,) int64 ascending positions in the fine sample_idx: the coarse samples
        sample_idx      fine.sample_idx[coarse]
        supp_edges      GeodesicSupportGraph(epsilon, max_num_neighbors=..., diagonals=...) on that preset sample
        logMag, logAng, xp, w       ComputeLogXPort(epsilon, diagonals=...)
        pool, unpool    the TransferPlans of level_transfer (fine -> coarse, coarse -> fine), cell weights from fine.w
        cell, n_outside every fine sample's cell (a position in coarse, -1: in no cell) and how many are in none
        interp          only with interpolate_k: the TransferPlan of interpolation_plan(k=interpolate_k, power=interpolate_power),
                        coarse -> fine from the k nearest coarse samples, which nn.TangentInterpolate takes; the mesh's edge graph
                        is then built once and shared with level_transfer

    so the coarse level is indistinguishable from a level built directly and FCPrecomp consumes it unchanged; nn.TangentPool and
    nn.TangentUnpool take it as their `level`.  The fine data is not modified.

    coarse=None selects min(n_coarse, S_f) samples, sorted ascending, by the rule `sampling` names; pass coarse to choose them
    yourself (it overrides either rule).
      'euclidean'   (the default) the Euclidean farthest-point sampling of the package over pos[sample_idx]
                    (farthest_point_sample, start 0).  Two sheets of a surface that pass close to each other in space may be
                    sampled as one at the coarse level.
      'geodesic'    geodesic_farthest_point_sample among the vertices sample_idx (candidates=sample_idx), started at the vertex
                    sample_idx[0], on the edge graph that diagonals= selects: the next coarse sample is the fine sample farthest,
                    over the surface, from those chosen; ties go to the lowest vertex number.  The taken vertices become
                    positions by torch.searchsorted(sample_idx, .).  The whole hierarchy is then intrinsic.
    The cells, the support edges and the transport are geodesic either way.  With 'geodesic' or interpolate_k the mesh's edge
    graph is built once and shared by the sampling, level_transfer and interpolation_plan.

    A fieldconv_amd.data.MeshBatch (pos_ptr and ptr present) goes through the batched launches (farthest_point_sample_batched
    over batch.ptr, or geodesic_farthest_point_sample_batched started at every mesh's first sample; min(n_coarse, n_b) samples
    per mesh) and yields a coarse MeshBatch with its own ptr, batch and edge_ptr; no cell crosses meshes: mesh for mesh what the
    single call gives.  With an explicit coarse on a batch give coarse_ptr too."""

    def __init__(self, n_coarse, epsilon, max_num_neighbors=512, diagonals=False, coarse=None, coarse_ptr=None, interpolate_k=None,
                 interpolate_power=2, sampling='euclidean'):
        what = 'CoarsenSamples'
        if sampling not in ('euclidean', 'geodesic'):
            raise ValueError(f"{what}: sampling must be 'euclidean' or 'geodesic', got {sampling!r}")
        self.sampling = sampling
        if coarse is None and (isinstance(n_coarse, bool) or n_coarse is None or int(n_coarse) != n_coarse or n_coarse < 1):
            raise ValueError(f'{what}: n_coarse must be an integer >= 1, got {n_coarse!r}')
        self.n_coarse = None if n_coarse is None else int(n_coarse)
        self.epsilon = _check_epsilon(epsilon, what)
        self.max_num_neighbors = _check_k(max_num_neighbors, what)
        if not isinstance(diagonals, bool):
            raise ValueError(f'{what}: diagonals must be True or False, got {diagonals!r}')
        self.diagonals = diagonals
        self.coarse, self.coarse_ptr = coarse, coarse_ptr
        self.interpolate_k = self.interpolate_power = None
        if interpolate_k is not None:
            self.interpolate_k, self.interpolate_power = _check_knn(interpolate_k, interpolate_power, what)

    def _select(self, data, batched, graph=None):
        """-> (coarse positions on pos's device, per-mesh counts or None); graph: the edge graph of the geodesic sampling"""
        from ..pooling import check_ptr, ptr_host
        pos = data.pos
        S_f = int(data.sample_idx.numel())
        if self.coarse is not None:
            _check_coarse(self.coarse, S_f, 'CoarsenSamples')
            counts = None
            if batched:
                if self.coarse_ptr is None:
                    raise ValueError('CoarsenSamples: an explicit coarse on a batch needs coarse_ptr, its ranges per mesh')
                hc = check_ptr(self.coarse_ptr, int(self.coarse.numel()), 'CoarsenSamples', 'coarse_ptr')
                counts = [b - a for a, b in zip(hc, hc[1:])]
            return self.coarse.to(pos.device), counts
        fine = data.sample_idx.to(pos.device)
        geodesic = self.sampling == 'geodesic'
        if not batched:
            if geodesic:
                taken = geodesic_farthest_point_sample(pos, data.face, min(self.n_coarse, S_f), int(fine[0]), graph=graph, candidates=fine)
                return torch.searchsorted(fine.contiguous(), taken).sort()[0], None
            return farthest_point_sample(pos[fine], min(self.n_coarse, S_f), 0).sort()[0], None
        hs = ptr_host(data.ptr, 'CoarsenSamples')
        n = [b - a for a, b in zip(hs, hs[1:])]
        if min(n) < 1:
            raise ValueError('CoarsenSamples: a mesh of the batch has no samples')
        counts = [min(self.n_coarse, v) for v in n]
        if geodesic:
            hp = ptr_host(data.pos_ptr, 'CoarsenSamples')
            first_vertex = fine[torch.tensor(hs[:-1], dtype=torch.int64, device=fine.device)].tolist()
            local = geodesic_farthest_point_sample_batched(pos, data.face, data.pos_ptr, counts, [v - o for v, o in zip(first_vertex, hp)],
                                                           graph=graph, candidates=fine, candidates_ptr=data.ptr)
            offset = torch.repeat_interleave(torch.tensor(hp[:-1], dtype=torch.int64), torch.tensor(counts, dtype=torch.int64))
            return torch.searchsorted(fine.contiguous(), local + offset.to(local.device)).sort()[0], counts
        local = farthest_point_sample_batched(pos[fine], data.ptr, counts, 0)
        first = torch.repeat_interleave(torch.tensor(hs[:-1], dtype=torch.int64), torch.tensor(counts, dtype=torch.int64))
        return (local + first.to(local.device)).sort()[0], counts          # (the ranges ascend with the mesh: one sort keeps the meshes apart)

    def __call__(self, data):
        for name in ('pos', 'face', 'sample_idx', 'w'):
            if getattr(data, name, None) is None:
                raise ValueError(f'CoarsenSamples: the fine level needs pos, face, sample_idx and w (run GeodesicSupportGraph and '
                                 f'ComputeLogXPort first); {name} is missing')
        pos = data.pos
        batched = getattr(data, 'pos_ptr', None) is not None
        if batched and getattr(data, 'ptr', None) is None:
            raise ValueError('CoarsenSamples: a batch needs ptr, the ranges of the sampled vertices')
        graph = None
        if self.interpolate_k is not None or (self.sampling == 'geodesic' and self.coarse is None):
            from ..geodesic import mesh_edge_graph
            graph = mesh_edge_graph(pos, data.face, self.diagonals)          # (the graph decides: diagonals stays False where it goes)
        coarse, counts = self._select(data, batched, graph)
        fine_idx = data.sample_idx.to(pos.device)
        if batched:
            from ..data.batch import MeshBatch
            out = MeshBatch()
            out.num_meshes = data.num_meshes
            out.pos, out.face, out.pos_ptr, out.face_ptr = pos, data.face, data.pos_ptr, getattr(data, 'face_ptr', None)
            out.sample_idx = fine_idx[coarse]
            out._set_ranges(counts, pos.device)
        else:
            out = SupportData(pos=pos, face=data.face, sample_idx=fine_idx[coarse])
        out.coarse = coarse
        out = GeodesicSupportGraph(self.epsilon, max_num_neighbors=self.max_num_neighbors, diagonals=self.diagonals)(out)
        out = ComputeLogXPort(self.epsilon, diagonals=self.diagonals)(out)
        ranges = dict(pos_ptr=data.pos_ptr if batched else None, ptr=data.ptr if batched else None, coarse_ptr=out.ptr if batched else None)
        which = dict(diagonals=self.diagonals) if graph is None else dict(graph=graph)
        out.pool, out.unpool, out.cell, out.n_outside = level_transfer(pos, data.face, fine_idx, coarse, data.w, return_cells=True, **which,
                                                                       **ranges)
        if self.interpolate_k is not None:
            out.interp = interpolation_plan(pos, data.face, fine_idx, coarse, self.interpolate_k, self.interpolate_power, graph=graph, **ranges)
        return out

    def __repr__(self):
        return '{}(n_coarse={}, epsilon={}, max_num_neighbors={}{}{}{})'.format(
            self.__class__.__name__, self.n_coarse, self.epsilon, self.max_num_neighbors, ', diagonals=True' if self.diagonals else '',
            ", sampling='geodesic'" if self.sampling == 'geodesic' else '',
            '' if self.interpolate_k is None else f', interpolate_k={self.interpolate_k}, interpolate_power={self.interpolate_power}')
