"""Host-side checks of geodesic sampling (fieldconv_amd.geodesic_sampling): the numpy restatement
tests/_geodesic_sampling_ref.py -- what the device is compared with exactly in tests/test_gpu_geodesic_sampling.py -- against
the plain multi-source Dijkstra after every round and against itself without the bound, the exported names, and the argument
checks (which run before anything is launched, so they need no device)."""
import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref


def _joined():
    pos, face, _ = gref.union([gref.lattice(9, 7), gref.surface(300, seed=1)])
    return pos, face


MESHES = {'lattice': lambda: gref.lattice(23, 17), 'surface': lambda: gref.surface(1500, seed=3), 'two_components': _joined}


@pytest.mark.parametrize('name', sorted(MESHES))
def test_incremental_field_is_the_multi_source_field_after_every_round(name):
    """the incremental start (keep the field, set d[new] = 0, lower from there) gives the bits of a Dijkstra from scratch
    over all the samples chosen so far, and the selection rule holds in every round"""
    pos, face = MESHES[name]()
    ptr, nbr, length = gref.edge_graph(pos, face)
    V = pos.shape[0]
    seen = []

    def check(k, idx, d):
        want = gref.dijkstra32(ptr, nbr, length, idx)
        assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), f'round {k}'
        seen.append(want.copy())

    idx, d = sref.fps(ptr, nbr, length, 64, start=5, each_round=check)
    assert idx[0] == 5 and len(set(idx.tolist())) == 64 and len(seen) == 64
    for k in range(63):          # idx[k+1]: the largest of the field before it among the vertices not taken, lowest number first
        free = np.setdiff1d(np.arange(V), idx[:k + 1])
        top = seen[k][free].max()
        assert idx[k + 1] == free[seen[k][free] == top][0]
    if name == 'two_components':
        assert idx[1] == 63 and np.isinf(seen[0][63:]).all()          # the other component comes first, at its lowest vertex
    assert np.isfinite(d).all()


def test_every_vertex_once_and_isolated_vertices_first():
    pos, face = sref.odd_mesh()
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert (length == 0).sum() == 2
    idx, d = sref.fps(ptr, nbr, length, 48, start=7)
    assert sorted(idx.tolist()) == list(range(48)) and (d == 0).all()
    assert idx[:3].tolist() == [7, 30, 46]          # +inf first, lowest number first: the second component, then the faceless vertex
    # vertex 47 lies on 14: once either is taken the other holds d = 0 and is still taken, last, with the other zeros
    assert abs(idx.tolist().index(14) - idx.tolist().index(47)) > 1


@pytest.mark.parametrize('name,epsilon', [('lattice', 0.375), ('surface', 0.2)])
def test_bounded_ball_edges_equal_the_thresholded_unbounded_ones(name, epsilon):
    pos, face = MESHES[name]()
    ptr, nbr, length = gref.edge_graph(pos, face)
    samples = np.sort(sref.fps(ptr, nbr, length, 64, start=5)[0])
    for k in (512, 4):
        e_full, d_full = sref.ball_edges(ptr, nbr, length, samples, epsilon, k)
        e_bound, d_bound = sref.ball_edges(ptr, nbr, length, samples, epsilon, k, bounded=True)
        assert np.array_equal(e_full, e_bound) and np.array_equal(d_full.view(np.uint32), d_bound.view(np.uint32))
        assert (np.bincount(e_full[:, 0], minlength=64) <= k).all() and (d_full < np.float32(epsilon)).all()
    e, d = sref.ball_edges(ptr, nbr, length, samples, epsilon)
    assert set(zip(range(64), range(64))) <= set(map(tuple, e.tolist())) and (d[e[:, 0] == e[:, 1]] == 0).all()
    assert np.array_equal(e, e[np.lexsort((e[:, 1], e[:, 0]))])          # grouped by query, neighbours ascending


# ------------------------------------------------------------------ the package's surface
NAMES = ['geodesic_farthest_point_sample', 'geodesic_farthest_point_sample_batched', 'geodesic_radius_edges']


def test_names_are_exported_and_bound():
    import fieldconv_amd.functional as F
    import fieldconv_amd.transforms as T
    from fieldconv_amd import _lib, build, geodesic_sampling
    from fieldconv_amd.transforms.geodesic_support_graph import GeodesicSupportGraph
    for name in NAMES:
        assert getattr(F, name) is getattr(geodesic_sampling, name)
        assert name in T.__all__ and getattr(T, name) is getattr(geodesic_sampling, name)
    assert 'GeodesicSupportGraph' in T.__all__ and T.GeodesicSupportGraph is GeodesicSupportGraph
    assert 'fc_geodesic_fps.hip' in build.SOURCES
    lib = _lib.load()
    cap = lib.fc_geodesic_fps_lds_vertices()
    assert cap == geodesic_sampling.LDS_VERTICES and 7 * cap + 1024 <= 160 * 1024          # sampling's 7 B per vertex fit the CU
    assert lib.fc_geodesic_fps_workspace_bytes(1000, 1000) == 0
    assert lib.fc_geodesic_fps_workspace_bytes(50000, cap + 1) == 3 * 50000
    assert lib.fc_geodesic_ball_workspace_bytes(cap, 100) == 0
    assert lib.fc_geodesic_ball_workspace_bytes(cap + 1, 100) >= 100 * 6 * (cap + 1)
    assert lib.fc_abi_version() == 11


def _mesh_t():
    pos, face = gref.lattice(4, 5)
    return torch.from_numpy(pos), torch.from_numpy(face)


def test_bad_arguments_raise_before_anything_runs():
    from fieldconv_amd import geodesic_sampling as G
    from fieldconv_amd.transforms import GeodesicSupportGraph
    from types import SimpleNamespace
    pos, face = _mesh_t()
    idx = torch.tensor([0, 7, 12], dtype=torch.int64)
    halves = torch.tensor([0, 10, 20], dtype=torch.int64)
    bad = [
        lambda: G.geodesic_farthest_point_sample(pos.double(), face, 4),                   # pos not float32
        lambda: G.geodesic_farthest_point_sample(pos, face.t().contiguous(), 4),            # (F,3): not the (3,F) layout
        lambda: G.geodesic_farthest_point_sample(pos, face, 0),
        lambda: G.geodesic_farthest_point_sample(pos, face, 21),                            # more samples than vertices
        lambda: G.geodesic_farthest_point_sample(pos, face, 2.5),
        lambda: G.geodesic_farthest_point_sample(pos, face, True),
        lambda: G.geodesic_farthest_point_sample(pos, face, 4, start=20),
        lambda: G.geodesic_farthest_point_sample(pos, face, 4, start=-1),
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, torch.tensor([0, 10, 19]), 4),            # does not end at V
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, [4, 11]),       # mesh 1 holds 10 vertices
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, [4, 4, 4]),     # three counts, two meshes
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 4, start=[0, 10]),               # start is local to the mesh
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, torch.tensor([0, 0, 20]), 1),            # an empty mesh
        lambda: G.geodesic_radius_edges(pos, face, torch.tensor([7, 0, 12]), 0.3),          # not ascending
        lambda: G.geodesic_radius_edges(pos, face, torch.tensor([0, 7, 7]), 0.3),           # not strictly
        lambda: G.geodesic_radius_edges(pos, face, torch.tensor([0, 20]), 0.3),             # index out of range
        lambda: G.geodesic_radius_edges(pos, face, torch.zeros(0, dtype=torch.int64), 0.3),
        lambda: G.geodesic_radius_edges(pos, face, idx.to(torch.int32), 0.3),
        lambda: G.geodesic_radius_edges(pos, face, idx, 0.0),
        lambda: G.geodesic_radius_edges(pos, face, idx, float('inf')),
        lambda: G.geodesic_radius_edges(pos, face, idx, 0.3, max_num_neighbors=0),
        lambda: G.geodesic_radius_edges(pos, face, idx, 0.3, pos_ptr=halves),                # one table without the other
        lambda: G.geodesic_radius_edges(pos, face, idx, 0.3, pos_ptr=halves, sample_ptr=torch.tensor([0, 3])),
        lambda: G.geodesic_radius_edges(pos, face, idx, 0.3, pos_ptr=halves, sample_ptr=torch.tensor([0, 1, 3])),       # vertex 7 is mesh 0's
        lambda: GeodesicSupportGraph(epsilon=-1.0),
        lambda: GeodesicSupportGraph(epsilon=0.2, sample_n=0),
        lambda: GeodesicSupportGraph(epsilon=0.2, max_num_neighbors=0),
        lambda: GeodesicSupportGraph(epsilon=0.2)(SimpleNamespace(pos=pos)),                 # no face
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {i} did not raise')
