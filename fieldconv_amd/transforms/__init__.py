from .fc_precomp import FCPrecomp
from .normalize import NormalizeArea, NormalizeAxes
from .precomp_cache import load_precomp, save_precomp
from .support_graph import (SupportGraph, farthest_point_sample, farthest_point_sample_batched, radius_edges,
                            radius_edges_batched)

__all__ = ['FCPrecomp', 'NormalizeArea', 'NormalizeAxes', 'SupportGraph', 'farthest_point_sample', 'load_precomp', 'radius_edges',
           'save_precomp', 'farthest_point_sample_batched', 'radius_edges_batched']
