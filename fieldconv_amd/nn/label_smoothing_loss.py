import torch.nn as nn

from ..losses import check_smoothing, label_smoothing_loss


class LabelSmoothingLoss(nn.Module):
    """Cross entropy against smoothed one-hot targets (reference nn/label_smoothing_loss.py): smoothing == 0 is the one-hot
    method, 0 < smoothing < 1 spreads smoothing / (classes - 1) over the other classes.  forward(pred (N,K), target (N)) with
    the class axis last (dim -1 or 1); one native launch each way."""

    def __init__(self, classes, smoothing=0.0, dim=-1, weight=None):
        super(LabelSmoothingLoss, self).__init__()
        check_smoothing(classes, smoothing)
        if dim not in (-1, 1):
            raise ValueError(f'LabelSmoothingLoss: pred is (N, classes) and dim must be -1 or 1, got {dim!r}')
        self.confidence = 1.0 - smoothing
        self.smoothing = smoothing
        self.weight = weight
        self.cls = classes
        self.dim = dim

    def forward(self, pred, target):
        if pred.dim() != 2:
            raise ValueError(f'LabelSmoothingLoss: pred must be (N, classes), got {tuple(pred.shape)}')
        return label_smoothing_loss(pred, target, self.cls, self.smoothing, self.weight)
