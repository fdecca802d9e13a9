"""Host-side checks of geodesic coarsening: the numpy restatement tests/_geodesic_coarsen_ref.py -- what the device is compared
with exactly in tests/test_gpu_geodesic_coarsen.py -- against the plain multi-source Dijkstra and the unrestricted restatement,
what it buys on a strip folded onto itself, the exported symbols, and the argument checks (which run before anything is
launched, so they need no device)."""
import numpy as np
import pytest
import torch

import _geodesic_coarsen_ref as cref
import _geodesic_ref as gref
import _geodesic_sampling_ref as sref


# ------------------------------------------------------------------ the restatement
def test_sampling_among_candidates_keeps_the_whole_field_and_the_rule():
    pos, face = gref.lattice(23, 17)
    ptr, nbr, length = gref.edge_graph(pos, face)
    cand = np.arange(0, pos.shape[0], 3)
    seen = []

    def check(k, idx, d, free):
        want = gref.dijkstra32(ptr, nbr, length, idx)          # over every vertex, candidate or not
        assert np.array_equal(d.view(np.uint32), want.view(np.uint32)), f'round {k}'
        seen.append((want.copy(), free.copy()))

    idx, _ = cref.fps_among(ptr, nbr, length, cand, 32, cand[2], each_round=check)
    assert idx[0] == cand[2] and len(set(idx.tolist())) == 32 and set(idx.tolist()) <= set(cand.tolist())
    for k in range(31):
        field, free = seen[k]
        assert np.array_equal(free, np.setdiff1d(cand, idx[:k + 1]))
        assert idx[k + 1] == free[field[free] == field[free].max()][0]
    # every vertex a candidate: the unrestricted sampling
    all_idx, all_d = cref.fps_among(ptr, nbr, length, np.arange(pos.shape[0]), 32, 5)
    want_idx, want_d = sref.fps(ptr, nbr, length, 32, 5)
    assert np.array_equal(all_idx, want_idx) and np.array_equal(all_d.view(np.uint32), want_d.view(np.uint32))


def test_ball_edges_at_is_the_filter_by_query():
    pos, face = gref.lattice(9, 7)
    samples = np.arange(0, 63, 4)
    edges, dist = sref.mesh_ball_edges(pos, face, samples, 0.375)
    some_e, some_d = cref.ball_edges_at(edges, dist, [1, 5, 6])
    assert set(some_e[:, 0].tolist()) == {1, 5, 6} and len(some_e) == sum((edges[:, 0] == q).sum() for q in (1, 5, 6))
    assert np.array_equal(some_d, dist[np.isin(edges[:, 0], [1, 5, 6])])


def test_folded_strip_is_two_sheets_a_gap_apart():
    pos, face = cref.folded_strip(41, 9, 0.125, 0.05)
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert pos.shape == (369, 3) and set(np.unique(pos[:, 2]).tolist()) == {0.0, float(np.float32(0.05))}
    assert np.isclose(length.min(), 0.05) and (np.isclose(length, 0.05).sum() == 2 * 9)          # one column of sides joins the sheets
    v = lambda i, j: i * 9 + j
    # the two ends of the strip face each other across the gap, a strip's length apart on the surface
    assert np.linalg.norm(pos[v(0, 4)] - pos[v(40, 4)]) < 0.14
    assert gref.dijkstra32(ptr, nbr, length, [v(0, 4)])[v(40, 4)] > 4.9


def test_geodesic_coarsening_covers_the_folded_strip_better():
    """the quality gate: 16 coarse samples of every second vertex of the folded strip; the geodesic covering radius (the largest
    edge-graph distance from a fine sample to its nearest coarse sample) of the geodesic choice is below the Euclidean one's"""
    pos, face = cref.folded_strip(41, 9, 0.125, 0.05)
    ptr, nbr, length = gref.edge_graph(pos, face)
    fine = np.arange(0, pos.shape[0], 2)
    assert len(fine) == 185
    geo = fine[cref.coarsen_geodesic(ptr, nbr, length, fine, 16)]
    euc = fine[cref.euclidean_fps(pos[fine], 16, 0)]
    assert len(set(geo.tolist())) == 16 and len(set(euc.tolist())) == 16
    r_geo, r_euc = cref.covering_radius(ptr, nbr, length, fine, geo), cref.covering_radius(ptr, nbr, length, fine, euc)
    print(f'folded strip 41 x 9, gap 0.05, 185 fine, 16 coarse: covering radius geodesic {r_geo:.4f}, Euclidean {r_euc:.4f}')
    assert r_geo < r_euc


# ------------------------------------------------------------------ the package's surface
SYMBOLS = ['fc_geodesic_fps_among', 'fc_geodesic_ball_count_at', 'fc_geodesic_ball_fill_at', 'fc_geodesic_fps_workspace_bytes',
           'fc_geodesic_ball_workspace_bytes']


def test_symbols_are_declared_bound_and_exported():
    """the three new entry points and the two size queries they reuse; the ABI version stays"""
    import os
    import re
    from fieldconv_amd import _lib, build
    with open(os.path.join(os.path.dirname(build.PKG), 'include', 'fieldconv_hip.h')) as f:
        declared = set(re.findall(r'\b(fc_\w+)\s*\(', f.read()))
    assert set(SYMBOLS) <= declared and set(SYMBOLS) <= set(_lib.SIGNATURES)
    assert [len(_lib.SIGNATURES[n][1]) for n in SYMBOLS[:3]] == [19, 21, 24]          # fps + mask, count / fill + (query_pos, Q)
    assert len(_lib.SIGNATURES['fc_geodesic_fps'][1]) == 18 and len(_lib.SIGNATURES['fc_geodesic_ball_count'][1]) == 19
    lib = _lib.load()
    for name in SYMBOLS:
        assert hasattr(lib, name)
    assert lib.fc_abi_version() == 11
    assert lib.fc_geodesic_fps_lds_vertices() == 20000
    # a null mask, a null list and an empty list are refused before anything is launched (every other pointer is a stand-in)
    one = 1 << 12
    assert lib.fc_geodesic_fps_among(one, one, one, 4, 6, None, 1, 4, None, one, one, one, 2, one, one, None, None, 0, None) == -1
    assert lib.fc_geodesic_ball_count_at(one, one, one, 4, 6, None, None, 1, 4, one, 2, None, 1, 0, 1, 0.5, 4, one, None, 0, None) == -1
    assert lib.fc_geodesic_ball_count_at(one, one, one, 4, 6, None, None, 1, 4, one, 2, one, 0, 0, 0, 0.5, 4, one, None, 0, None) == -1
    assert lib.fc_geodesic_ball_count_at(one, one, one, 4, 6, None, None, 1, 4, one, 2, one, 3, 2, 2, 0.5, 4, one, None, 0, None) == -1


def _mesh_t():
    pos, face = gref.lattice(4, 5)
    return torch.from_numpy(pos), torch.from_numpy(face)


def test_bad_arguments_raise_before_anything_runs():
    from fieldconv_amd import geodesic_sampling as G
    from fieldconv_amd.transforms import CoarsenSamples
    pos, face = _mesh_t()
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    cand = t(0, 3, 7, 12, 19)
    halves = t(0, 10, 20)
    both = t(0, 3, 7, 12, 19)          # mesh 0: 0 3 7, mesh 1: 12 19
    cptr = t(0, 3, 5)
    samples = t(0, 7, 12)
    bad = [
        lambda: G.geodesic_farthest_point_sample(pos, face, 3, candidates=t(3, 0, 7)),                        # not ascending
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, candidates=t(0, 3, 3)),                        # not strictly
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, candidates=t(0, 3, 20)),                       # out of range
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, candidates=t(-1, 3)),
        lambda: G.geodesic_farthest_point_sample(pos, face, 1, candidates=t()),                               # none
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, candidates=cand.to(torch.int32)),
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, candidates=[0, 3, 7]),
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, start=1, candidates=cand),                     # start is no candidate
        lambda: G.geodesic_farthest_point_sample(pos, face, 2, start=13, candidates=cand),
        lambda: G.geodesic_farthest_point_sample(pos, face, 6, candidates=cand),                              # five candidates
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates_ptr=cptr),  # a table without candidates
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=both),      # candidates without a table
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=both, candidates_ptr=t(0, 5, 5)),   # a mesh with none (and mesh 0 holds mesh 1's)
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 1, [0, 2], candidates=t(0, 3, 7), candidates_ptr=t(0, 3, 3)),   # a mesh with none
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=both, candidates_ptr=t(0, 4, 5)),   # vertex 12 is mesh 1's
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=both, candidates_ptr=t(0, 3, 4)),   # does not end at M
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=both, candidates_ptr=t(0, 5)),      # one mesh, two meshes
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 2], candidates=t(0, 7, 3, 12, 19), candidates_ptr=cptr),   # not ascending
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [0, 3], candidates=both, candidates_ptr=cptr),   # start 13 is no candidate
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, 2, [1, 2], candidates=both, candidates_ptr=cptr),
        lambda: G.geodesic_farthest_point_sample_batched(pos, face, halves, [3, 3], [0, 2], candidates=both, candidates_ptr=cptr),   # mesh 1 has two
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(1, 0)),                            # not ascending
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(1, 1)),
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(0, 3)),                            # three samples
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(-1, 0)),
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(0, 1).to(torch.int32)),
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=[0, 1]),
        lambda: G.geodesic_radius_edges(pos, face, samples, 0.3, queries=t(0, 1).reshape(2, 1)),
        lambda: G.geodesic_radius_edges(pos, face, t(7, 0, 12), 0.3, queries=t()),                            # the other checks come first
        lambda: CoarsenSamples(4, 0.5, sampling='intrinsic'),
        lambda: CoarsenSamples(4, 0.5, sampling=None),
        lambda: CoarsenSamples(4, 0.5, sampling=True),
    ]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {i} did not raise')
    # the good neighbours of the cases above pass their checks and stop at the device (a machine without one) or run
    assert CoarsenSamples(4, 0.5).sampling == 'euclidean' and CoarsenSamples(4, 0.5, sampling='geodesic').sampling == 'geodesic'
    assert "sampling='geodesic'" in repr(CoarsenSamples(4, 0.5, sampling='geodesic')) and 'sampling' not in repr(CoarsenSamples(4, 0.5))


def test_no_queries_give_no_rows_without_a_device():
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face = _mesh_t()
    samples = torch.tensor([0, 7, 12], dtype=torch.int64)
    none = torch.zeros(0, dtype=torch.int64)
    edges = geodesic_radius_edges(pos, face, samples, 0.3, queries=none)
    assert tuple(edges.shape) == (0, 2) and edges.dtype == torch.int64
    edges, dist = geodesic_radius_edges(pos, face, samples, 0.3, queries=none, return_dist=True)
    assert tuple(edges.shape) == (0, 2) and tuple(dist.shape) == (0,) and dist.dtype == torch.float32
