"""data.w of the reference's data contract (what its computeLogXPort takes from fcutils.weights): every sampled vertex's share
of the surface, the lumped vertex masses summed onto each vertex's geodesically nearest sample.  Computed on the ROCm device
by fieldconv_amd.geodesic (the edge-graph metric, not fcutils' heat method); the result stays on data.pos's device."""
from ..geodesic import sample_weights


class SampleWeights(object):
    """Sets data.w (S,1) float32 from data.pos (V,3) float32, data.face (3,F) and data.sample_idx (S,) -- run it after
    SupportGraph.  A fieldconv_amd.data.MeshBatch (pos_ptr and ptr present) is handled in one launch, every mesh's vertices
    searching their own mesh's samples only: mesh for mesh what the single-mesh call gives.
    diagonals=True finds the nearest samples over mesh_edge_graph(pos, face, diagonals=True); graph: such a graph already built
    (then diagonals stays False: the graph decides)."""

    def __init__(self, diagonals=False, graph=None):
        if not isinstance(diagonals, bool):
            raise ValueError(f'SampleWeights: diagonals must be True or False, got {diagonals!r}')
        if diagonals and graph is not None:
            raise ValueError('SampleWeights: graph= already decides which edges there are; leave diagonals at False')
        self.diagonals, self.graph = diagonals, graph

    def __call__(self, data):
        if getattr(data, 'sample_idx', None) is None or getattr(data, 'face', None) is None:
            raise ValueError('SampleWeights: data needs pos, face and sample_idx (run SupportGraph first)')
        if getattr(data, 'pos_ptr', None) is not None:
            if getattr(data, 'ptr', None) is None:
                raise ValueError('SampleWeights: a batch needs ptr, the ranges of the sampled vertices')
            data.w = sample_weights(data.pos, data.face, data.sample_idx.to(data.pos.device), data.pos_ptr, data.ptr, graph=self.graph,
                                    diagonals=self.diagonals)
        else:
            data.w = sample_weights(data.pos, data.face, data.sample_idx.to(data.pos.device), graph=self.graph, diagonals=self.diagonals)
        return data

    def __repr__(self):
        return '{}({})'.format(self.__class__.__name__, 'diagonals=True' if self.diagonals else '')
