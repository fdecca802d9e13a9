import torch.nn as nn

from ..losses import twin_eval


class TwinEval(nn.Module):
    """forward(xS, xT, p_, n_) -> (nFN, nFP) Python ints: the positive pairs farther apart than mu * ratio (false negatives)
    and the negative pairs closer than it (false positives), as the reference's nn/twin_eval.py counts them.  n_ = None stands
    for every pair that is not in p_, counted without building that list."""

    def __init__(self, mu=5, ratio=0.5):
        super(TwinEval, self).__init__()
        self.mu = mu          # Matching threshold value
        self.ratio = ratio

    def forward(self, xS, xT, p_, n_=None):
        return twin_eval(xS, xT, p_, n_, self.mu * self.ratio)
