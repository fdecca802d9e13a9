"""Host-side checks of the mesh geodesics (fieldconv_amd.geodesic): the numpy float32 restatement tests/_geodesic_ref.py --
what the device is compared with bit for bit in tests/test_gpu_geodesic.py -- against scipy's float64 Dijkstra and against
itself under another relaxation order, the exported names, and the argument checks (which run before anything is launched,
so they need no device)."""
import numpy as np
import pytest
import torch

import _geodesic_ref as gref

MESHES = {'lattice': lambda: gref.lattice(13, 13), 'surface': lambda: gref.surface(400, seed=1)}


@pytest.fixture(scope='module', params=sorted(MESHES))
def mesh(request):
    pos, face = MESHES[request.param]()
    return (pos, face) + gref.edge_graph(pos, face)


def test_restated_distances_match_scipy_float64(mesh):
    """float32 additions along a path of h hops are off by at most h * 2^-24 relative (all terms positive); the paths of
    these meshes have fewer than 100 hops: 6e-6 < 1e-5"""
    import scipy.sparse as sp
    from scipy.sparse.csgraph import dijkstra
    pos, face, ptr, nbr, length = mesh
    V = pos.shape[0]
    # (a zero-length entry would be dropped by the sparse format; these two meshes have none)
    assert (length > 0).all()
    graph = sp.csr_matrix((length.astype(np.float64), nbr, ptr), shape=(V, V))
    sources = gref.spread(V, 9)
    for s in sources[:4]:
        want = dijkstra(graph, indices=int(s))
        got = gref.dijkstra32(ptr, nbr, length, [s])
        assert got.dtype == np.float32 and np.isfinite(got).all()
        assert np.max(np.abs(got - want) / np.maximum(want, 1e-30)) <= 1e-5
    want = dijkstra(graph, indices=sources, min_only=True)
    got = gref.dijkstra32(ptr, nbr, length, sources)
    assert np.max(np.abs(got - want)[want > 0] / want[want > 0]) <= 1e-5


def test_random_order_sweeps_reach_the_same_bits_and_labels(mesh):
    pos, face, ptr, nbr, length = mesh
    V = pos.shape[0]
    sources = gref.spread(V, 9)
    d = gref.dijkstra32(ptr, nbr, length, sources)
    label = gref.tight_labels(ptr, nbr, length, d, sources)
    for seed in (0, 1):
        rng = np.random.default_rng(seed)
        d_sweep, sweeps = gref.sweep_distances(ptr, nbr, length, sources, rng)
        assert sweeps > 1 and np.array_equal(d_sweep.view(np.uint32), d.view(np.uint32))
        assert np.array_equal(gref.tight_labels(ptr, nbr, length, d_sweep, sources, rng=rng), label)
    assert label.min() >= 0 and set(label[sources]) == set(range(9)) and np.array_equal(label[sources], np.arange(9))


def test_lattice_has_vertices_whose_tight_predecessors_disagree():
    """the case a one-phase (distance, label) propagation would resolve by schedule"""
    pos, face = gref.lattice(13, 13)
    ptr, nbr, length = gref.edge_graph(pos, face)
    sources = gref.spread(169, 9)
    d = gref.dijkstra32(ptr, nbr, length, sources)
    label = gref.tight_labels(ptr, nbr, length, d, sources)
    assert gref.tied_vertices(ptr, nbr, length, d, label)


def test_restated_edge_graph_and_weights():
    pos, face = gref.surface(400, seed=1)
    ptr, nbr, length = gref.edge_graph(pos, face)
    rows = gref.slot_rows(ptr)
    assert all(np.all(np.diff(nbr[ptr[v]:ptr[v + 1]]) > 0) for v in range(400))           # ascending, no duplicates
    pairs = set(zip(rows.tolist(), nbr.tolist()))
    assert all((b, a) in pairs for a, b in pairs) and len(pairs) == len(nbr)
    sides = {(int(face[i, f]), int(face[j, f])) for f in range(face.shape[1]) for i in range(3) for j in range(3) if i != j}
    assert pairs == sides
    label, _ = gref.nearest(pos, face, gref.spread(400, 9))
    w = gref.sample_weights(pos, face, label, 9)
    assert w.shape == (9, 1) and w.dtype == np.float32
    assert abs(float(w.astype(np.float64).sum()) - gref.area64(pos, face)) <= 1e-6 * gref.area64(pos, face)


# ------------------------------------------------------------------ the package's surface
NAMES = ['mesh_edge_graph', 'geodesic_distances', 'nearest_sample', 'samples_to_nearest', 'compose_map', 'sample_weights',
         'geodesic_error', 'correspondence_curve']


def test_names_are_exported_and_bound():
    import fieldconv_amd.functional as F
    import fieldconv_amd.transforms as T
    import fieldconv_amd.utils as U
    from fieldconv_amd import _lib, geodesic
    for name in NAMES:
        assert getattr(F, name) is getattr(geodesic, name)
    for name in ('SampleWeights', 'sample_weights', 'nearest_sample', 'geodesic_distances', 'mesh_edge_graph'):
        assert name in T.__all__ and hasattr(T, name)
    for name in ('samples_to_nearest', 'compose_map', 'geodesic_error', 'correspondence_curve'):
        assert name in U.__all__ and getattr(U, name) is getattr(geodesic, name)
    lib = _lib.load()
    assert lib.fc_geodesic_lds_vertices() == geodesic.LDS_VERTICES
    assert 8 * geodesic.LDS_VERTICES + 256 <= 160 * 1024          # distances, labels and the reduction's static scratch fit the CU
    assert lib.fc_geodesic_workspace_bytes(1000, 1000) == 0
    assert lib.fc_geodesic_workspace_bytes(50000, geodesic.LDS_VERTICES + 1) == 4 * 50000


def _mesh_t():
    pos, face = gref.lattice(4, 5)
    return torch.from_numpy(pos), torch.from_numpy(face)


def test_bad_arguments_raise_before_anything_runs():
    from fieldconv_amd import geodesic as G
    pos, face = _mesh_t()
    idx = torch.tensor([0, 7], dtype=torch.int64)
    ok_ptr = torch.tensor([0, 20], dtype=torch.int64)
    bad = [
        lambda: G.mesh_edge_graph(pos.double(), face),                                   # pos not float32
        lambda: G.mesh_edge_graph(pos[:, :2], face),
        lambda: G.mesh_edge_graph(pos, face.t().contiguous()),                            # (F,3): not the (3,F) layout
        lambda: G.mesh_edge_graph(pos, face.to(torch.int32)),
        lambda: G.geodesic_distances(pos, face, torch.tensor([0, 20])),                  # index out of range
        lambda: G.geodesic_distances(pos, face, torch.tensor([-1])),
        lambda: G.geodesic_distances(pos, face, torch.zeros(0, dtype=torch.int64)),      # empty sources
        lambda: G.geodesic_distances(pos, face, idx, rows_per_call=0),
        lambda: G.geodesic_distances(pos, face, idx.to(torch.int32)),
        lambda: G.nearest_sample(pos, face, torch.zeros(0, dtype=torch.int64)),
        lambda: G.nearest_sample(pos, face, torch.tensor([20])),
        lambda: G.nearest_sample(pos, face, idx, pos_ptr=ok_ptr),                        # one table without the other
        lambda: G.nearest_sample(pos, face, idx, pos_ptr=torch.tensor([0, 19]), sample_ptr=torch.tensor([0, 2])),
        lambda: G.nearest_sample(pos, face, idx, pos_ptr=torch.tensor([0, 10, 20]), sample_ptr=torch.tensor([0, 2, 2])),     # a mesh without samples
        lambda: G.nearest_sample(pos, face, idx, pos_ptr=torch.tensor([0, 10, 20]), sample_ptr=torch.tensor([0, 2])),
        lambda: G.samples_to_nearest(pos, face, torch.tensor([0.5])),
        lambda: G.compose_map(torch.tensor([3, 4]), torch.tensor([0, 1]), pos, face),    # 1-based labels: 0 is out of range
        lambda: G.compose_map(torch.tensor([3, 4]), torch.tensor([1, 21]), pos, face),
        lambda: G.compose_map(torch.tensor([3, 4, 5]), torch.tensor([1, 2]), pos, face),
        lambda: G.sample_weights(pos, face, torch.tensor([20])),
        lambda: G.geodesic_error(pos, face, torch.tensor([0, 1]), torch.tensor([0, 20])),
        lambda: G.geodesic_error(pos, face, torch.tensor([0]), torch.tensor([0, 1])),
        lambda: G.correspondence_curve(torch.zeros(0), [0.1]),
        lambda: G.correspondence_curve(torch.zeros(3, dtype=torch.int64), [0.1]),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {i} did not raise')


def test_correspondence_curve_is_plain_torch():
    from fieldconv_amd.geodesic import correspondence_curve
    err = torch.tensor([0.0, 0.05, 0.1, 0.2, float('inf'), float('nan')])
    got = correspondence_curve(err, [0.0, 0.1, 0.15, 1.0])
    assert got.dtype == torch.float64 and got.tolist() == [1 / 6, 3 / 6, 3 / 6, 4 / 6]
