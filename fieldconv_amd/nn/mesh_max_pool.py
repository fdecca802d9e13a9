import torch.nn as nn

from ..pooling import mesh_max


class MeshMaxPool(nn.Module):
    """Per-mesh max read-out of a mini-batch of meshes (a MeshBatch): forward(x (N,C), ptr (B+1)) -> (B,C) real, row b the softAbs of
    the entry of largest magnitude among mesh b's rows ptr[b] .. ptr[b+1] - 1 for complex features (soft_abs=True), or the plain
    max of x for real ones (soft_abs=False); ties go to the first row.  pooling.mesh_max: two native launches forward, one
    backward, bitwise repeatable; an empty mesh gives 0; only the winning row of a (mesh, channel) receives a gradient."""

    def __init__(self, soft_abs=True):
        super(MeshMaxPool, self).__init__()
        self.soft_abs = bool(soft_abs)

    def forward(self, x, ptr):
        return mesh_max(x, ptr, self.soft_abs, False, 'MeshMaxPool')

    def extra_repr(self):
        return 'soft_abs={}'.format(self.soft_abs)
