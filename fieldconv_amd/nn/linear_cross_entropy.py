import torch

from ..head import linear_cross_entropy, linear_topk


class LinearCrossEntropy(torch.nn.Linear):
    """The classification head `Linear(in_features, n_classes)` + cross-entropy as ONE device op (fieldconv_amd.head): the
    (N, n_classes) logits are never built.  A torch.nn.Linear by parameters -- .weight (K,H), .bias (K), the same names and
    initialisation -- so the state_dict of the reference's `lin2` loads into it.  smoothing as in LabelSmoothingLoss."""

    def __init__(self, in_features, n_classes, bias=True, smoothing=0.0, ignore_index=-100, reduction='mean'):
        super().__init__(in_features, n_classes, bias=bias)
        self.smoothing, self.ignore_index, self.reduction = float(smoothing), int(ignore_index), reduction

    def forward(self, h, target, parts=0):
        return linear_cross_entropy(h, self.weight, self.bias, target, self.reduction, self.smoothing, self.ignore_index, parts)

    def predict(self, h, k=1, parts=0):
        """(idx (N,k) int64, z (N,k)): the k classes with the largest logits per row and those logits (linear_topk)"""
        return linear_topk(h, self.weight, self.bias, k, parts)

    def extra_repr(self):
        return super().extra_repr() + f', smoothing={self.smoothing}, reduction={self.reduction!r}'
