"""CPU tests of the support-graph preprocessing (fieldconv_amd.transforms): the public names, the mesh normalisers against
float64 numpy, and argument checks that fire before any device work."""
import math

import numpy as np
import pytest
import torch


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def icosphere(subdiv):
    """Unit icosphere: vertices (V,3) float64, faces (F,3) int64 (outward orientation)."""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
         (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.array(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = verts[a] + verts[b]
                verts.append(p / np.linalg.norm(p))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(verts), np.array(f, dtype=np.int64)


def mesh_area64(p, f):
    a, b, c = p[f[:, 0]], p[f[:, 1]], p[f[:, 2]]
    return 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()


def test_public_names_import_from_transforms():
    from fieldconv_amd import transforms
    from fieldconv_amd.transforms import (NormalizeArea, NormalizeAxes, SupportGraph, farthest_point_sample,  # noqa: F401
                                          radius_edges)
    for name in ('NormalizeArea', 'NormalizeAxes', 'SupportGraph', 'farthest_point_sample', 'radius_edges'):
        assert name in transforms.__all__
    # the convolution's internal graph class keeps its own name and module
    from fieldconv_amd.graph import SupportGraph as InternalGraph
    assert InternalGraph is not SupportGraph


def test_normalize_area_matches_float64():
    from fieldconv_amd.transforms import NormalizeArea
    v, f = icosphere(3)
    # an ellipsoid moved off the origin: the area is no longer 4 pi, the bounding box not centred
    v = v * np.array([1.5, 0.7, 2.2]) + np.array([0.3, -1.2, 4.0])
    pos = torch.from_numpy(v.astype(np.float32))
    d = NormalizeArea()(Data(pos=pos.clone(), face=torch.from_numpy(f.T.copy())))
    p32 = v.astype(np.float32).astype(np.float64)
    c = p32 - (p32.max(0) + p32.min(0)) / 2
    ref = c / math.sqrt(mesh_area64(c, f))
    assert d.pos.dtype == torch.float32 and d.pos.shape == pos.shape
    assert np.max(np.abs(d.pos.numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
    # the result has unit area
    assert abs(mesh_area64(d.pos.numpy().astype(np.float64), f) - 1.0) < 1e-5


def cuboid(a, b, c, n):
    """Closed triangulated box [0,a] x [0,b] x [0,c], each face an n x n grid: vertices (V,3), faces (F,3); area 2(ab+bc+ca)."""
    verts, index, faces = [], {}, []

    def vid(p):
        key = tuple(np.round(p, 12))
        if key not in index:
            index[key] = len(verts)
            verts.append(p)
        return index[key]
    ext = np.array([a, b, c], dtype=np.float64)
    for axis in range(3):
        u, w = [k for k in range(3) if k != axis]
        for side in (0.0, 1.0):
            for i in range(n):
                for j in range(n):
                    quad = []
                    for di, dj in ((0, 0), (1, 0), (1, 1), (0, 1)):
                        p = np.zeros(3)
                        p[axis] = side * ext[axis]
                        p[u] = (i + di) / n * ext[u]
                        p[w] = (j + dj) / n * ext[w]
                        quad.append(vid(p))
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.array(verts), np.array(faces, dtype=np.int64)


def test_normalize_area_of_a_known_mesh():
    """A closed box of sides (2, 1, 0.5): area 7 exactly, so the scale is 1 / sqrt(7) and the box is centred."""
    from fieldconv_amd.transforms import NormalizeArea
    v, f = cuboid(2.0, 1.0, 0.5, 4)
    assert abs(mesh_area64(v, f) - 7.0) < 1e-12
    d = NormalizeArea()(Data(pos=torch.from_numpy(v.astype(np.float32)), face=torch.from_numpy(f.T.copy())))
    ref = (v - np.array([1.0, 0.5, 0.25])) / math.sqrt(7.0)
    assert np.max(np.abs(d.pos.numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
    assert abs(mesh_area64(d.pos.numpy().astype(np.float64), f) - 1.0) < 1e-5


@pytest.mark.parametrize('perm', [(0, 1, 2), (2, 0, 1), (1, 2, 0), (2, 1, 0)])
@pytest.mark.parametrize('scale', [True, False])
def test_normalize_axes_matches_float64(perm, scale):
    from fieldconv_amd.transforms import NormalizeAxes
    rng = np.random.default_rng(3)
    base = rng.standard_normal((500, 3)) * np.array([0.2, 1.0, 3.0])         # std ascending by construction
    v = base[:, list(perm)].astype(np.float32)
    d = NormalizeAxes(normalize_scale=scale)(Data(pos=torch.from_numpy(v.copy())))
    v64 = v.astype(np.float64)
    order = np.argsort(v64.std(0, ddof=1), kind='stable')
    ref = v64[:, order]
    if scale:
        ref = ref / (2 * ref[:, 2].max())
    assert d.pos.dtype == torch.float32
    assert np.max(np.abs(d.pos.numpy() - ref)) <= 1e-6 * np.max(np.abs(ref))
    # the original axes come back in ascending-spread order whatever the permutation
    inv = np.argsort(perm)
    assert list(order) == list(inv)


def test_bad_arguments_raise_before_device_work(monkeypatch):
    from fieldconv_amd.transforms import SupportGraph, farthest_point_sample, radius_edges
    from fieldconv_amd import _lib

    def no_device(*a, **k):
        raise AssertionError('device work attempted')
    monkeypatch.setattr(_lib, 'load', no_device)
    pos = torch.rand(10, 3)
    for eps in (0.0, -1.0, float('nan'), float('inf'), 1e-50):         # (1e-50 is 0 in float32)
        with pytest.raises(ValueError):
            radius_edges(pos, eps)
        with pytest.raises(ValueError):
            SupportGraph(eps)
    for k in (0, -3, 1.5):
        with pytest.raises(ValueError):
            radius_edges(pos, 0.1, max_num_neighbors=k)
    for bad in (torch.rand(10, 2), torch.rand(10), torch.rand(2, 10, 3), torch.rand(0, 3), np.zeros((4, 3))):
        with pytest.raises(ValueError):
            radius_edges(bad, 0.1)
        with pytest.raises(ValueError):
            farthest_point_sample(bad, 1)
        with pytest.raises(ValueError):
            SupportGraph(0.1)(Data(pos=bad))
    for s in (0, -1, 11, 2.5):
        with pytest.raises(ValueError):
            farthest_point_sample(pos, s)
    for start in (-1, 10):
        with pytest.raises(ValueError):
            farthest_point_sample(pos, 3, start=start)
    for s in (0, -5):
        with pytest.raises(ValueError):
            SupportGraph(0.1, sample_n=s)
