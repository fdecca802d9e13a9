"""computeLogXPort of the reference's preprocessing chain, on the ROCm device: data.xp, data.logMag, data.logAng by the discrete
exponential map of fieldconv_amd.logmap (the edge-graph metric; not fcutils' Vector Heat Method, no parity with it claimed) and
data.w by SampleWeights.  Results stay on data.pos's device."""
from ..geodesic import mesh_edge_graph
from ..logmap import _check_bound, log_map_transport
from .sample_weights import SampleWeights


class ComputeLogXPort(object):
    """Sets data.logMag (E,), data.logAng (E,) float32 and data.xp (E,) complex64 for the rows of data.supp_edges, and data.w
    (S,1), from data.pos, data.face, data.sample_idx and data.supp_edges -- run it after SupportGraph or GeodesicSupportGraph.
    bound: how far each sample's shortest-path tree is grown; pass the support graph's epsilon.  After
    GeodesicSupportGraph(epsilon) every target is inside its source's tree; after the Euclidean SupportGraph a target further
    than bound along the surface falls back to the tangent-plane projection of the chord (log_map_transport).
    A fieldconv_amd.data.MeshBatch (pos_ptr and ptr present) is handled in one launch per kernel, every query inside its own
    mesh: mesh for mesh what the single-mesh call gives.
    diagonals=True grows the trees, and finds data.w's nearest samples, over mesh_edge_graph(pos, face, diagonals=True); after
    GeodesicSupportGraph(epsilon, diagonals=True) every target is again inside its source's tree."""

    def __init__(self, bound, diagonals=False):
        self.bound = _check_bound(bound, 'ComputeLogXPort')
        if not isinstance(diagonals, bool):
            raise ValueError(f'ComputeLogXPort: diagonals must be True or False, got {diagonals!r}')
        self.diagonals = diagonals

    def __call__(self, data):
        for name in ('pos', 'face', 'sample_idx', 'supp_edges'):
            if getattr(data, name, None) is None:
                raise ValueError(f'ComputeLogXPort: data needs pos, face, sample_idx and supp_edges (run SupportGraph first); {name} is missing')
        pos = data.pos
        pos_ptr, ptr = getattr(data, 'pos_ptr', None), getattr(data, 'ptr', None)
        if pos_ptr is not None and ptr is None:
            raise ValueError('ComputeLogXPort: a batch needs ptr, the ranges of the sampled vertices')
        if pos_ptr is None:
            ptr = None
        graph = mesh_edge_graph(pos, data.face, self.diagonals)
        data.logMag, data.logAng, data.xp = log_map_transport(pos, data.face, data.sample_idx.to(pos.device), data.supp_edges.to(pos.device),
                                                              self.bound, graph=graph, pos_ptr=pos_ptr, ptr=ptr)
        return SampleWeights(graph=graph)(data)

    def __repr__(self):
        return '{}(bound={}{})'.format(self.__class__.__name__, self.bound, ', diagonals=True' if self.diagonals else '')


computeLogXPort = ComputeLogXPort
