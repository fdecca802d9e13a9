"""A coarser sample level of a mesh and the two transfers that join it to the fine one: what an encoder / decoder needs to
change resolution inside a network.  Built on the ROCm device from the package's own pieces (farthest-point sampling,
GeodesicSupportGraph, ComputeLogXPort, fieldconv_amd.transfer.level_transfer); results stay on data.pos's device, the two plans
on the ROCm device."""
import torch

from ..data.synthetic import SupportData
from ..transfer import _check_coarse, _check_knn, interpolation_plan, level_transfer
from .compute_log_xport import ComputeLogXPort
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

    coarse=None selects min(n_coarse, S_f) samples by the Euclidean farthest-point sampling of the package over pos[sample_idx]
    (farthest_point_sample, start 0, sorted ascending); pass coarse to choose them yourself.  A geodesic farthest-point sampling
    restricted to a candidate subset of the vertices does not exist in the package and is out of scope here: two sheets of a
    surface that pass close to each other in space may therefore be sampled as one at the coarse level; the cells, the support
    edges and the transport are geodesic either way.

    A fieldconv_amd.data.MeshBatch (pos_ptr and ptr present) goes through the batched launches (farthest_point_sample_batched
    over batch.ptr, min(n_coarse, n_b) samples per mesh) and yields a coarse MeshBatch with its own ptr, batch and edge_ptr; no
    cell crosses meshes: mesh for mesh what the single call gives.  With an explicit coarse on a batch give coarse_ptr too."""

    def __init__(self, n_coarse, epsilon, max_num_neighbors=512, diagonals=False, coarse=None, coarse_ptr=None, interpolate_k=None,
                 interpolate_power=2):
        what = 'CoarsenSamples'
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

    def _select(self, data, batched):
        """-> (coarse positions on pos's device, per-mesh counts or None)"""
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
        pts = pos[data.sample_idx.to(pos.device)]
        if not batched:
            return farthest_point_sample(pts, min(self.n_coarse, S_f), 0).sort()[0], None
        hs = ptr_host(data.ptr, 'CoarsenSamples')
        n = [b - a for a, b in zip(hs, hs[1:])]
        if min(n) < 1:
            raise ValueError('CoarsenSamples: a mesh of the batch has no samples')
        counts = [min(self.n_coarse, v) for v in n]
        local = farthest_point_sample_batched(pts, data.ptr, counts, 0)
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
        coarse, counts = self._select(data, batched)
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
        if self.interpolate_k is None:
            out.pool, out.unpool, out.cell, out.n_outside = level_transfer(pos, data.face, fine_idx, coarse, data.w, diagonals=self.diagonals,
                                                                           return_cells=True, **ranges)
            return out
        from ..geodesic import mesh_edge_graph
        graph = mesh_edge_graph(pos, data.face, self.diagonals)          # (the graph decides: diagonals stays False below)
        out.pool, out.unpool, out.cell, out.n_outside = level_transfer(pos, data.face, fine_idx, coarse, data.w, graph=graph, return_cells=True,
                                                                       **ranges)
        out.interp = interpolation_plan(pos, data.face, fine_idx, coarse, self.interpolate_k, self.interpolate_power, graph=graph, **ranges)
        return out

    def __repr__(self):
        return '{}(n_coarse={}, epsilon={}, max_num_neighbors={}{}{})'.format(
            self.__class__.__name__, self.n_coarse, self.epsilon, self.max_num_neighbors, ', diagonals=True' if self.diagonals else '',
            '' if self.interpolate_k is None else f', interpolate_k={self.interpolate_k}, interpolate_power={self.interpolate_power}')
