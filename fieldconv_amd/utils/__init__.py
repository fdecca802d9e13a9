from .field import EPS, isZero, isOrigin, softAbs, softAngle, softAbsolute, softSqrt

from .step_graph import StepGraph
from .pairs import hard_null_pairs, null_pair_count, null_pairs_from_rank, sample_null_pairs, twin_eval_curve
from ..geodesic import compose_map, correspondence_curve, geodesic_error, samples_to_nearest

__all__ = ['StepGraph', 'null_pair_count', 'null_pairs_from_rank', 'sample_null_pairs', 'twin_eval_curve', 'hard_null_pairs', 'compose_map', 'correspondence_curve', 'geodesic_error', 'samples_to_nearest', 'EPS', 'isZero', 'isOrigin', 'softAbs', 'softAngle', 'softAbsolute', 'softSqrt']
