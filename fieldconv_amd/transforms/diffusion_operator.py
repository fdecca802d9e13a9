"""data.diffusion_plan: the stiffness matrix of a sample level's connection Laplacian (fieldconv_amd.diffusion), built on the ROCm
device from what ComputeLogXPort leaves on data."""
from ..diffusion import _check_h, diffusion_plan


class DiffusionOperator(object):
    """Sets data.diffusion_plan, the DiffusionPlan of diffusion_plan(data.supp_edges, data.xp, data.logMag, S, data.w, h), S the
    number of samples -- run it after ComputeLogXPort.  data.w (S,1) is used when present (flattened), else every mass is 1.
    nn.TangentDiffusion and functional.heat_diffuse take the plan.  A fieldconv_amd.data.MeshBatch is a union graph whose rows
    never cross meshes, so the plan of a batch is, mesh for mesh, the plan of the single call GIVEN THE SAME h: with h=None the
    batch's width comes from the largest active logMag of the whole batch; pass h= for the single calls' bits."""

    def __init__(self, h=None):
        self.h = _check_h(h, 'DiffusionOperator')

    def __call__(self, data):
        for name in ('sample_idx', 'supp_edges', 'logMag', 'xp'):
            if getattr(data, name, None) is None:
                raise ValueError(f'DiffusionOperator: data needs sample_idx, supp_edges, logMag and xp (run ComputeLogXPort first); '
                                 f'{name} is missing')
        dev = data.logMag.device
        w = getattr(data, 'w', None)
        data.diffusion_plan = diffusion_plan(data.supp_edges.to(dev), data.xp.to(dev), data.logMag, int(data.sample_idx.numel()),
                                             None if w is None else w.to(dev).reshape(-1), self.h)
        return data

    def __repr__(self):
        return '{}(h={})'.format(self.__class__.__name__, self.h)
