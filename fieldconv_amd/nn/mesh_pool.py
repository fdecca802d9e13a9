import torch.nn as nn

from ..pooling import mesh_pool


class MeshPool(nn.Module):
    """Per-mesh read-out of a mini-batch of meshes (a MeshBatch): forward(x (N,C), ptr (B+1)) -> (B,C) real, row b the mean
    (reduce='mean') or sum (reduce='sum') over mesh b's vertices ptr[b] .. ptr[b+1] - 1 of softAbs(x) for complex features
    (soft_abs=True: the classification networks' `mean(softAbs(x), dim=0)`, one row per mesh) or of x itself for real ones
    (soft_abs=False).  Two native launches forward, one backward, bitwise repeatable; an empty mesh gives 0."""

    def __init__(self, reduce='mean', soft_abs=True):
        super(MeshPool, self).__init__()
        if reduce not in ('mean', 'sum'):
            raise ValueError(f"MeshPool: reduce must be 'mean' or 'sum', got {reduce!r}")
        self.reduce = reduce
        self.soft_abs = bool(soft_abs)

    def forward(self, x, ptr):
        return mesh_pool(x, ptr, self.reduce, self.soft_abs, 'MeshPool')

    def extra_repr(self):
        return 'reduce={!r}, soft_abs={}'.format(self.reduce, self.soft_abs)
