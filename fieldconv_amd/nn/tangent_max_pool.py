import torch.nn as nn

from ..transfer import tangent_transfer_max


class TangentMaxPool(nn.Module):
    """forward(x (S_f,C), level) -> (S_c,C): max pooling of a fine level's features onto the coarse `level` built by
    transforms.CoarsenSamples (any object with a .pool TransferPlan).  Per coarse sample and channel the ONE member of its cell with
    the largest magnitude -- key fl(fl(re * re) + fl(im * im)), which does not depend on a sample's frame; ties go to the member
    listed first -- parallel-transported into the coarse sample's frame.  Real features take the plain max of the cell, bit for bit.
    The plan's weights are not read: every member of a cell counts alike.  A fine sample in no cell is ignored, an empty cell gives
    zero, and the gradient of every member that did not win is exactly zero.  Equals tangent_transfer_max(x, level.pool): one
    native launch forward and one backward, bitwise repeatable.  No parameters."""

    def forward(self, x, level):
        return tangent_transfer_max(x, level.pool)
