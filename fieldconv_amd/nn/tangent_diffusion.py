import torch
import torch.nn as nn

from ..diffusion import heat_diffuse


class TangentDiffusion(nn.Module):
    """forward(x (n,C), plan, ptr=None) -> (n,C): learned heat diffusion y = (I - t L)^-1 x with one diffusion time per channel
    (diffusion.heat_diffuse), L the connection Laplacian of a DiffusionPlan built by transforms.DiffusionOperator
    (data.diffusion_plan) or diffusion.diffusion_plan.  A global, resolution-robust receptive field that commutes with any change
    of the samples' frames; complex (tangent) and real features are both accepted, in single or double precision.

    channels   C
    iters      conjugate-gradient steps of the solve (and of its adjoint in the backward pass), 1 .. 1024
    init_time  the initial diffusion time of every channel, or a (channels,) sequence

    One parameter, `time` (channels,) float32, used as time.clamp(min=0): a channel can learn to switch diffusion off, and
    stays there bit for bit (t = 0 returns x).  ptr is a MeshBatch.ptr.  One native launch forward, at most four backward."""

    def __init__(self, channels, iters=16, init_time=1e-3):
        super().__init__()
        self.channels, self.iters = int(channels), int(iters)
        if self.channels < 1 or not 1 <= self.iters <= 1024:
            raise ValueError(f'TangentDiffusion: channels >= 1 and iters in [1, 1024], got {channels}, {iters}')
        init = torch.as_tensor(init_time, dtype=torch.float32)
        if init.dim() == 0:
            init = init.repeat(self.channels)
        if tuple(init.shape) != (self.channels,) or not bool(torch.isfinite(init).all()) or bool((init < 0).any()):
            raise ValueError(f'TangentDiffusion: init_time must be a number >= 0 or ({self.channels},) of them, got {init_time!r}')
        self.time = nn.Parameter(init.clone())

    def forward(self, x, plan, ptr=None):
        real = x.real.dtype if x.is_complex() else x.dtype
        return heat_diffuse(x, self.time.clamp(min=0).to(real), plan, ptr=ptr, iters=self.iters)

    def extra_repr(self):
        return 'channels={}, iters={}'.format(self.channels, self.iters)
