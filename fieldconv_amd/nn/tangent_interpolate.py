import torch.nn as nn

from ..transfer import tangent_transfer


class TangentInterpolate(nn.Module):
    """forward(x (S_c,C), level) -> (S_f,C): the features of the coarse `level` (any object with an .interp TransferPlan, as
    transforms.CoarsenSamples(..., interpolate_k=k) builds it) interpolated onto the fine samples: per fine sample the
    inverse-distance-weighted combination of its k nearest coarse samples, every tangent-vector feature parallel-transported
    into the fine sample's frame first; real features take the weights alone.  The smooth counterpart of TangentUnpool, which
    is constant over each cell; a coarse sample keeps its own value exactly.  One native launch forward and one backward,
    bitwise repeatable.  No parameters."""

    def forward(self, x, level):
        return tangent_transfer(x, level.interp)
