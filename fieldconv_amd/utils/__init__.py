from .field import EPS, isZero, isOrigin, softAbs, softAngle, softAbsolute, softSqrt

from .step_graph import StepGraph
from .pairs import hard_null_pairs, null_pair_count, null_pairs_from_rank, sample_null_pairs, twin_eval_curve

__all__ = ['StepGraph', 'null_pair_count', 'null_pairs_from_rank', 'sample_null_pairs', 'twin_eval_curve', 'hard_null_pairs', 'EPS', 'isZero', 'isOrigin', 'softAbs', 'softAngle', 'softAbsolute', 'softSqrt']
