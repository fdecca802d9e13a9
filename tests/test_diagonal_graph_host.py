"""The numpy restatement of the edge graph with unfolded diagonals (tests/_diagonal_graph_ref.py) tested on its own: the
hand-made meshes, the layout of the CSR, and what the diagonals buy on the unit icosphere.  No device needed."""
import functools

import numpy as np
import pytest

import _diagonal_graph_ref as dref
import _geodesic_ref as gref
import _geodesic_sampling_ref as sref
import _logmap_ref as lref

F32 = np.float32


def gained(mesh):
    """{(lo, hi): length} of the undirected pairs the enriched graph has and the side graph has not, and the two graphs"""
    pos, face = mesh
    side, rich = dref.pairs_of(*gref.edge_graph(pos, face)), dref.pairs_of(*dref.edge_graph(pos, face))
    assert set(side) <= set(rich)
    return {p: l for p, l in rich.items() if p not in side and p[0] < p[1]}, side, rich


def test_square_gains_the_other_diagonal():
    new, side, rich = gained(dref.square())
    assert list(new) == [(1, 3)]
    assert new[(1, 3)].dtype == F32 and new[(1, 3)] == np.sqrt(F32(2))
    assert rich[(3, 1)] == new[(1, 3)]
    assert all(rich[p] == side[p] for p in side)          # the sides keep their lengths


def test_concave_quad_gains_nothing():
    pos, face = dref.concave()
    assert dref.unfold(pos, 0, 2, 1, 3) is None          # t = 2 lies beyond L = 1
    new, side, rich = gained((pos, face))
    assert not new and rich.keys() == side.keys()


@pytest.mark.parametrize('mesh', ['single', 'fan3', 'twice', 'degenerate', 'zero_side'])
def test_no_diagonal_from(mesh):
    """boundary sides, a side of three faces, one face listed twice (c == d), a face that names a vertex twice, and a shared side
    of length zero: each leaves exactly the side graph"""
    pos, face = getattr(dref, mesh)()
    assert dref.candidates(pos, face) == []
    ptr, nbr, length = dref.edge_graph(pos, face)
    sptr, snbr, slen = gref.edge_graph(pos, face)
    assert np.array_equal(ptr, sptr) and np.array_equal(nbr, snbr) and np.array_equal(length.view(np.uint32), slen.view(np.uint32))


def test_a_degenerate_face_does_not_count_for_its_side():
    new, _, _ = gained(dref.square_with_degenerate())
    assert list(new) == [(1, 3)] and new[(1, 3)] == np.sqrt(F32(2))


def test_pair_reached_from_several_sides_keeps_the_minimum():
    pos, face = dref.octahedron()
    cands = dref.candidates(pos, face)
    apex = [ln for lo, hi, ln, _ in cands if (lo, hi) == (0, 1)]
    assert len(apex) == 4 and len(set(float(x) for x in apex)) == 4          # the four equator sides, four lengths
    new, side, rich = gained((pos, face))
    assert (0, 1) not in side and new[(0, 1)] == min(apex) and rich[(1, 0)] == min(apex)
    for pair in ((2, 4), (3, 5)):                                            # opposite equator vertices: across two sides of each apex
        ways = [ln for lo, hi, ln, _ in cands if (lo, hi) == pair]
        assert len(ways) == 4 and len(set(float(x) for x in ways)) > 1 and new[pair] == min(ways)


@pytest.mark.parametrize('mesh', ['joined', 'ico', 'grid', 'two'])
def test_rows_ascend_and_are_symmetric_in_bits(mesh):
    pos, face = {'joined': lambda: dref.joined()[:2], 'ico': lambda: lref.icosphere(2), 'grid': lambda: lref.jittered_grid(9, 7),
                 'two': lref.two_components}[mesh]()
    ptr, nbr, length = dref.edge_graph(pos, face)
    V = pos.shape[0]
    assert ptr.shape == (V + 1,) and ptr[0] == 0 and ptr[-1] == len(nbr) == len(length) and length.dtype == F32
    rows = gref.slot_rows(ptr)
    assert (rows != nbr).all()
    for v in range(V):
        assert (np.diff(nbr[ptr[v]:ptr[v + 1]]) > 0).all()
    pairs = dref.pairs_of(ptr, nbr, length)
    assert len(pairs) == len(nbr)
    assert all(pairs[(b, a)].view(np.uint32) == l.view(np.uint32) for (a, b), l in pairs.items())
    side = dref.pairs_of(*gref.edge_graph(pos, face))
    assert set(side) <= set(pairs) and all(pairs[p] <= side[p] for p in side)
    if mesh != 'joined':
        assert len(pairs) > len(side)


def test_union_has_no_diagonal_across_meshes():
    pos, face, pos_ptr = dref.joined()
    ptr, nbr, length = dref.edge_graph(pos, face)
    parts = [dref.edge_graph(*m()) for m in dref.HAND_MADE]
    assert np.array_equal(nbr, np.concatenate([p[1] + o for p, o in zip(parts, pos_ptr[:-1])]))
    assert np.array_equal(length.view(np.uint32), np.concatenate([p[2] for p in parts]).view(np.uint32))
    assert np.array_equal(np.diff(ptr), np.concatenate([np.diff(p[0]) for p in parts]))


def test_accuracy_on_the_icosphere():
    """Dijkstra in float64 against the great-circle distance on icosphere(3), 41 sources, pairs more than 0.2 apart: the mean
    excess with diagonals is at most a third of the side graph's, and no distance is 6 % too long.
    Measured: side graph mean 1.0652 max 1.2296; with diagonals mean 1.0123 max 1.0445 (0.19 of the mean excess)."""
    pos, face = lref.icosphere(3)
    side = dref.sphere_accuracy(pos, *gref.edge_graph(pos, face))
    rich = dref.sphere_accuracy(pos, *dref.edge_graph(pos, face))
    print(f'\nicosphere(3), d / true: side graph mean {side[0]:.4f} max {side[1]:.4f}; with diagonals mean {rich[0]:.4f} max {rich[1]:.4f}')
    assert rich[0] - 1 <= (side[0] - 1) / 3
    assert rich[1] < 1.06


@functools.lru_cache(maxsize=None)
def ico_case_with_diagonals():
    """lref.ico_case's recipe on the enriched graph: 128 geodesic FPS samples, the balls of ICO_BOUND"""
    pos, face = lref.icosphere(3)
    graph = dref.edge_graph(pos, face)
    samples = np.sort(sref.fps(*graph, 128, 0)[0])
    edges, _ = sref.ball_edges(*graph, samples, lref.ICO_BOUND)
    return dref.GraphCase(pos, face, samples, edges, lref.ICO_BOUND)


def test_log_map_on_both_graphs_against_the_closed_form_sphere():
    """not gated: how the float64 log map's distance to the closed-form sphere moves when its trees grow over the enriched graph
    (logMag relative, logAng and arg(xp) in radians, each the maximum over the rows; the rows differ: each graph has its own
    samples and balls)"""
    side, rich = lref.ico_case(), ico_case_with_diagonals()
    a = lref.closed_form_errors(side, *side.values(np.float64))
    b = lref.closed_form_errors(rich, *rich.values(np.float64))
    print(f'\nlog map against the closed form (logMag rel, logAng rad, arg(xp) rad): side graph {len(side.edges)} rows '
          f'{a[0]:.4f} {a[1]:.4f} {a[2]:.4f}; with diagonals {len(rich.edges)} rows {b[0]:.4f} {b[1]:.4f} {b[2]:.4f}')
    assert rich.reached.all() and np.isfinite(b).all()
