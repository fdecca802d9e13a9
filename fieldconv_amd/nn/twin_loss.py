import torch
import torch.nn as nn

from ..losses import twin_loss


## Twin loss for source + target features (reference nn/twin_loss.py; Supplement C, Equation (5))

class TwinLoss(nn.Module):
    """forward(xS, xT, p_, n_) -> (1,) tensor in the features' dtype: mean squared distance of the positive pairs p_, plus
    for the negative pairs n_ the mean of yN d2 + (1 - yN) max(mu - d2, 0) with yN = 0.2 torch.rand(M) drawn here on the
    features' device (torch's generator: torch.manual_seed governs it).  Pair rows are [row of xT, row of xS].  One native
    launch forward and one backward (fieldconv_amd.losses.twin_loss); no host synchronisation, so a step with this loss
    replays in a StepGraph."""

    def __init__(self, mu=5):
        super(TwinLoss, self).__init__()
        self.mu = mu

    def forward(self, xS, xT, p_, n_):
        if not (torch.is_tensor(xS) and xS.is_cuda):
            raise RuntimeError('TwinLoss: features must be on a ROCm device; fieldconv_amd has no CPU path')
        yN = 0.2 * torch.rand(n_.size(0), device=xS.device).float()
        return twin_loss(xS, xT, p_, n_, yN, self.mu)
