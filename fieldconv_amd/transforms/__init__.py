from .fc_precomp import FCPrecomp
from .normalize import NormalizeArea, NormalizeAxes
from .precomp_cache import load_precomp, save_precomp
from .sample_weights import SampleWeights
from .support_graph import (SupportGraph, farthest_point_sample, farthest_point_sample_batched, radius_edges,
                            radius_edges_batched)
from ..geodesic import geodesic_distances, mesh_edge_graph, nearest_sample, sample_weights
from ..geodesic_sampling import (geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched, geodesic_radius_edges)
from .geodesic_support_graph import GeodesicSupportGraph
from ..logmap import log_map_transport, vertex_frames
from .compute_log_xport import ComputeLogXPort, computeLogXPort
from .coarsen_samples import CoarsenSamples
from .samples_to_vertices import SamplesToVertices
from .random_mesh_affine import RandomMeshAffine
from .gradient_operator import GradientOperator
from .diffusion_operator import DiffusionOperator

__all__ = ['FCPrecomp', 'NormalizeArea', 'NormalizeAxes', 'SupportGraph', 'farthest_point_sample', 'load_precomp', 'radius_edges',
           'save_precomp', 'farthest_point_sample_batched', 'radius_edges_batched', 'SampleWeights', 'geodesic_distances',
           'mesh_edge_graph', 'nearest_sample', 'sample_weights', 'GeodesicSupportGraph', 'geodesic_farthest_point_sample',
           'geodesic_farthest_point_sample_batched', 'geodesic_radius_edges', 'ComputeLogXPort', 'computeLogXPort', 'log_map_transport',
           'vertex_frames', 'CoarsenSamples', 'SamplesToVertices', 'RandomMeshAffine', 'GradientOperator', 'DiffusionOperator']
