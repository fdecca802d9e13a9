"""Mesh normalisers of the reference's preprocessing chain (NormalizeArea, NormalizeAxes).  One-shot O(V + F) reductions:
plain torch on whatever device data.pos is on."""
import torch


class NormalizeArea(object):
    """Centres data.pos on the midpoint of its bounding box, then scales it to unit surface area: by 1 / sqrt(total area of
    the triangles data.face (3,F)), the area summed in float64."""

    def __call__(self, data):
        pos = data.pos
        pos = pos - (pos.max(dim=0)[0] + pos.min(dim=0)[0]) / 2
        p = pos.to(torch.float64)
        f = data.face.to(device=pos.device, dtype=torch.long)
        a, b, c = p[f[0]], p[f[1]], p[f[2]]
        area = 0.5 * torch.linalg.cross(b - a, c - a, dim=1).norm(dim=1).sum()
        data.pos = pos * (1.0 / area.sqrt()).to(pos.dtype)
        return data

    def __repr__(self):
        return '{}()'.format(self.__class__.__name__)


class NormalizeAxes(object):
    """Reorders the axes of data.pos by ascending (unbiased) standard deviation; with normalize_scale, then scales by
    1 / (2 * the largest coordinate on the new third axis)."""

    def __init__(self, normalize_scale=True):
        self.normalize_scale = normalize_scale

    def __call__(self, data):
        pos = data.pos
        order = torch.sort(torch.std(pos, dim=0), stable=True)[1]
        pos = pos[:, order]
        if self.normalize_scale:
            pos = pos * (1 / (2 * pos[:, 2].max()))
        data.pos = pos
        return data

    def __repr__(self):
        return '{}(normalize_scale={})'.format(self.__class__.__name__, self.normalize_scale)
