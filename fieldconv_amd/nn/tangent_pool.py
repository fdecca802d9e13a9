import torch.nn as nn

from ..transfer import tangent_transfer


class TangentPool(nn.Module):
    """forward(x (S_f,C), level) -> (S_c,C): the features of a fine level pooled onto the coarse `level` built by
    transforms.CoarsenSamples (any object with a .pool TransferPlan): per coarse sample the mass-weighted mean of its cell, every
    tangent-vector feature parallel-transported into the coarse sample's frame first; real features take the weights alone.  One
    native launch forward and one backward, bitwise repeatable.  No parameters."""

    def forward(self, x, level):
        return tangent_transfer(x, level.pool)


class TangentUnpool(nn.Module):
    """forward(x (S_c,C), level) -> (S_f,C): the features of the coarse `level` (any object with an .unpool TransferPlan) carried
    out to the fine samples of each cell, transported into their frames; a fine sample in no cell gets zero.  The adjoint
    direction of TangentPool up to the cell weights: TangentPool(TangentUnpool(y)) = y.  No parameters."""

    def forward(self, x, level):
        return tangent_transfer(x, level.unpool)
