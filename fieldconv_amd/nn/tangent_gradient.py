import torch.nn as nn

from ..diffops import tangent_divergence, tangent_gradient


class TangentGradient(nn.Module):
    """forward(x (n,C) real, plan) -> (n,C) complex: the intrinsic gradient of every channel as a tangent-vector feature in each
    sample's frame (diffops.tangent_gradient), for a GradientPlan built by transforms.GradientOperator (data.grad_plan) or
    diffops.gradient_plan.  A parameter-free, gauge-equivariant lift from scalar to tangent features: applied to
    pos[sample_idx] it gives three tangent channels without a LiftBlock.  One native launch forward and one backward, bitwise
    repeatable.  No parameters."""

    def forward(self, x, plan):
        return tangent_gradient(x, plan)


class TangentDivergence(nn.Module):
    """forward(x (n,C) complex, plan) -> (n,C) real: the divergence of every tangent-vector channel (diffops.tangent_divergence),
    the negative adjoint of TangentGradient in the inner products weighted by plan.w: a parameter-free, gauge-invariant read-out
    from tangent features back to scalars.  One native launch forward and one backward, bitwise repeatable.  No parameters."""

    def forward(self, x, plan):
        return tangent_divergence(x, plan)
