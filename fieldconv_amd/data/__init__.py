from .synthetic import random_support, sphere_partition, sphere_support
from .batch import MeshBatch

__all__ = ['random_support', 'sphere_support', 'sphere_partition', 'MeshBatch']
