"""data.grad_plan: the sparse intrinsic gradient of a sample level (fieldconv_amd.diffops), built on the ROCm device from what
ComputeLogXPort leaves on data."""
from ..diffops import RCOND, _check_rcond, gradient_plan


class GradientOperator(object):
    """Sets data.grad_plan, the GradientPlan of gradient_plan(data.supp_edges, data.logMag, data.logAng, S, data.w, rcond), S the
    number of samples -- run it after ComputeLogXPort.  data.w (S,1) is used when present (flattened), else every weight is 1.
    nn.TangentGradient, nn.TangentDivergence and functional.laplacian take the plan.  A fieldconv_amd.data.MeshBatch is a union
    graph whose rows never cross meshes, so the plan of a batch is, mesh for mesh, the plan of the single call."""

    def __init__(self, rcond=RCOND):
        self.rcond = _check_rcond(rcond, 'GradientOperator')

    def __call__(self, data):
        for name in ('sample_idx', 'supp_edges', 'logMag', 'logAng'):
            if getattr(data, name, None) is None:
                raise ValueError(f'GradientOperator: data needs sample_idx, supp_edges, logMag and logAng (run ComputeLogXPort first); '
                                 f'{name} is missing')
        dev = data.logMag.device
        w = getattr(data, 'w', None)
        data.grad_plan = gradient_plan(data.supp_edges.to(dev), data.logMag, data.logAng, int(data.sample_idx.numel()),
                                       None if w is None else w.to(dev).reshape(-1), self.rcond)
        return data

    def __repr__(self):
        return '{}(rcond={})'.format(self.__class__.__name__, self.rcond)
