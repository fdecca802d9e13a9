import torch
import torch.nn as nn

from ..norm import tangent_norm


class TangentNorm(nn.Module):
    """Per-mesh normalisation of tangent features: forward(x (N,C) complex, ptr=None, w=None) -> (N,C), every channel of every
    mesh (the rows ptr[b] .. ptr[b+1] - 1; the whole tensor without ptr) scaled by gain[c] / sqrt(m[b,c] + eps), m the mean of
    |x|^2 over the mesh's rows, weighted by the integration weights w (data.w) when given.  No mean is subtracted -- a mean over
    samples would mix their frames -- so the layer touches magnitudes only and commutes with any change of frames.  No running
    statistics: training and evaluation compute the same thing.

        x = TangentNorm(48)(conv(x, e, s), batch.ptr, batch.w)

    gain (1,channels), ones at the start (TangentNonLin.bias's shape); affine=False has no parameter.  Three native launches
    forward, at most four backward, bitwise repeatable (fieldconv_amd.norm.tangent_norm)."""

    def __init__(self, channels, eps=1e-5, affine=True):
        super().__init__()
        if isinstance(channels, bool) or int(channels) != channels or channels < 1:
            raise ValueError(f'TangentNorm: channels must be a positive integer, got {channels!r}')
        if isinstance(eps, bool) or not float(eps) >= 0:
            raise ValueError(f'TangentNorm: eps must be a number >= 0, got {eps!r}')
        self.channels, self.eps, self.affine = int(channels), float(eps), bool(affine)
        if self.affine:
            self.gain = nn.Parameter(torch.ones(1, self.channels))
        else:
            self.register_parameter('gain', None)

    def forward(self, x, ptr=None, w=None):
        return tangent_norm(x, self.gain, ptr, w, self.eps)

    def extra_repr(self):
        return '{}, eps={}, affine={}'.format(self.channels, self.eps, self.affine)
