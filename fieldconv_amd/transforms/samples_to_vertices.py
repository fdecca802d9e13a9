"""data.to_vertices: the plan that carries per-sample features to every vertex of the mesh (fieldconv_amd.transfer.
vertex_interpolation), for a full-resolution read-out of a network that runs on the samples.  Built on the ROCm device; the
plan stays there."""
from ..logmap import _check_bound
from ..transfer import _check_knn, vertex_interpolation


class SamplesToVertices(object):
    """Sets data.to_vertices, the TransferPlan (V x S) of vertex_interpolation(pos, face, sample_idx, k, power, radius), from
    data.pos, data.face and data.sample_idx (S,) strictly ascending -- run it after SupportGraph or GeodesicSupportGraph.
    tangent_transfer(x, data.to_vertices) then gives every vertex the inverse-distance-weighted combination of its k nearest
    samples: logits and other real features by the weights alone, tangent features transported into the vertex's frame.  A
    fieldconv_amd.data.MeshBatch (pos_ptr and ptr present) goes through the batched path: no row crosses meshes, mesh for mesh
    what the single call gives.  diagonals=True measures over mesh_edge_graph(pos, face, diagonals=True)."""

    def __init__(self, k=3, power=2, radius=None, diagonals=False):
        what = 'SamplesToVertices'
        self.k, self.power = _check_knn(k, power, what)
        self.radius = None if radius is None else _check_bound(radius, what)
        if not isinstance(diagonals, bool):
            raise ValueError(f'{what}: diagonals must be True or False, got {diagonals!r}')
        self.diagonals = diagonals

    def __call__(self, data):
        if getattr(data, 'sample_idx', None) is None or getattr(data, 'face', None) is None:
            raise ValueError('SamplesToVertices: data needs pos, face and sample_idx (run SupportGraph first)')
        batched = getattr(data, 'pos_ptr', None) is not None
        if batched and getattr(data, 'ptr', None) is None:
            raise ValueError('SamplesToVertices: a batch needs ptr, the ranges of the sampled vertices')
        data.to_vertices = vertex_interpolation(data.pos, data.face, data.sample_idx.to(data.pos.device), self.k, self.power, self.radius,
                                                diagonals=self.diagonals, pos_ptr=data.pos_ptr if batched else None,
                                                ptr=data.ptr if batched else None)
        return data

    def __repr__(self):
        return '{}(k={}, power={}{}{})'.format(self.__class__.__name__, self.k, self.power, '' if self.radius is None else f', radius={self.radius}',
                                               ', diagonals=True' if self.diagonals else '')
