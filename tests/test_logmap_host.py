"""The numpy restatement of the discrete-exponential-map log map (tests/_logmap_ref.py) against what can be known without a
device: a planar mesh (the unfolding is exact there: signs and the direction of xp), the closed-form sphere of
fieldconv_amd.data.synthetic (the method's discretisation error, printed), a mesh whose tight edges are cyclic (the tree is
not), and the argument checks of the Python layer, which come before any device is needed."""
import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref
import _logmap_ref as lref
from _logmap_ref import ICO_BOUND, closed_form_errors, ico_case

def test_planar_grid_unfolds_exactly():
    pos, face = lref.jittered_grid(9, 9)
    S = pos.shape[0]
    case = lref.Case(pos, face, np.arange(S), lref.all_pairs(S), 0.6)
    assert case.reached.any() and not case.reached.all()          # rows inside and beyond the bound: both rules
    L, X = case.values(np.float64)
    n, e1, e2 = lref.frames(pos, face, np.float64)
    assert np.array_equal(n, np.tile([0.0, 0.0, 1.0], (S, 1)))
    disp = pos[case.edges[:, 1]].astype(np.float64) - pos[case.edges[:, 0]].astype(np.float64)
    a = case.edges[:, 0]
    want = np.stack(((disp * e1[a]).sum(1), (disp * e2[a]).sum(1)), 1)
    # the frame (e1, e2, n) is right-handed and the same everywhere: transport is the identity, the path's edges add up to the displacement
    assert np.abs(X - np.array([1.0, 0.0])).max() < 1e-14
    assert np.abs(L - want).max() < 1e-13 * np.abs(want).max() + 1e-15
    assert np.array_equal(np.cross(e1, e2), n)
    # a conjugated or inverted convention would show here: the row [a, b] points from a to b
    mag, ang = lref.polar(L)
    r = int(np.nonzero((a == 40) & (case.edges[:, 1] == 41))[0][0])          # the next vertex along +y: e1 = -y, so the angle is pi
    assert abs(abs(ang[r]) - np.pi) < 0.5 and abs(mag[r] - np.linalg.norm(disp[r])) < 1e-12


def test_icosphere_against_the_closed_form():
    case = ico_case()
    assert case.reached.all() and 15 < len(case.edges) / 128 < 25
    L, X = case.values(np.float64)
    mag, ang, xp = closed_form_errors(case, L, X)
    print(f'\ndiscretisation error of the float64 restatement on the 642-vertex icosphere, 128 samples, bound {ICO_BOUND}: '
          f'logMag {mag:.3e} relative, logAng {ang:.3e} rad, arg(xp) {xp:.3e} rad')
    # Not a tolerance on the method, only that it is the same map: the unfolded path ends within one mesh cell of the geodesic's
    # end (edges of this icosphere subtend about 0.16 rad, the nearest sample pairs lie about 0.3 apart).
    assert mag < 0.5 and ang < 0.5 and xp < 0.5


def test_tree_is_acyclic_where_tight_edges_are_not():
    pos, face = lref.two_components()
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert length[ptr[47] + np.searchsorted(nbr[ptr[47]:ptr[48]], 14)] == 0          # the zero-length edge
    for source in (0, 14, 47, 29, 35):
        d = lref.bounded_field(ptr, nbr, length, source, 10.0)
        assert d[14] == d[47]          # each is a tight predecessor of the other
        h, pred = lref.tree(ptr, nbr, length, d, source)
        assert np.array_equal(h >= 0, np.isfinite(d)) and h[source] == 0 and pred[source] == -1
        for v in np.nonzero(h > 0)[0]:
            assert h[pred[v]] == h[v] - 1          # so every chain of predecessors ends at the source after h[v] steps
        assert (h[46] < 0) and ((h[30:46] >= 0).all() if 30 <= source < 46 else (h[30:46] < 0).all())


def test_float32_restatement_stays_near_float64():
    case = ico_case()
    (L32, X32), (L64, X64) = case.values(np.float32), case.values(np.float64)
    assert L32.dtype == np.float32 and np.abs(L32 - L64).max() < 1e-5 and np.abs(X32 - X64).max() < 1e-5


def test_arguments_are_checked_before_any_device_is_needed():
    from fieldconv_amd.logmap import log_map_transport, vertex_frames
    from fieldconv_amd.transforms import ComputeLogXPort, computeLogXPort
    assert computeLogXPort is ComputeLogXPort
    pos, face = (torch.from_numpy(a) for a in lref.jittered_grid(4, 4))
    idx = torch.arange(16)
    edges = torch.tensor([[0, 1], [2, 3]])
    bad = [
        dict(pos=pos.double()), dict(face=face.int()), dict(face=face.t().contiguous()), dict(sample_idx=idx.int()),
        dict(sample_idx=torch.tensor([0, 16])), dict(supp_edges=edges.float()), dict(supp_edges=edges[:, :1]), dict(supp_edges=torch.tensor([[0, 16]])),
        dict(supp_edges=torch.tensor([[-1, 0]])), dict(bound=0.0), dict(bound=float('nan')), dict(bound='x'), dict(pos_ptr=torch.tensor([0, 16])),
        dict(ptr=torch.tensor([0, 16])), dict(pos_ptr=torch.tensor([0, 8, 16]), ptr=torch.tensor([0, 16])),
        dict(pos_ptr=torch.tensor([0, 8, 16]), ptr=torch.tensor([0, 4, 16])), dict(ball_lds_vertices=1025), dict(ball_lds_vertices=-1),
    ]
    for change in bad:
        kw = dict(pos=pos, face=face, sample_idx=idx, supp_edges=edges, bound=0.5)
        kw.update(change)
        with pytest.raises(ValueError):
            log_map_transport(**kw)
    with pytest.raises(ValueError):
        log_map_transport(torch.zeros(8192, 3), face, torch.arange(4096), edges, 0.5, return_tree=True)          # not a small case
    with pytest.raises(ValueError):
        vertex_frames(pos.double(), face)
    for b in (0, -1.0, float('inf'), None):
        with pytest.raises(ValueError):
            ComputeLogXPort(b)
    from types import SimpleNamespace
    with pytest.raises(ValueError):
        ComputeLogXPort(0.5)(SimpleNamespace(pos=pos, face=face, sample_idx=idx))          # no supp_edges


def test_entry_points_are_declared_bound_and_built():
    import os
    import re
    from fieldconv_amd import _lib, build
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', open(os.path.join(root, 'include', 'fieldconv_hip.h')).read()))
    names = {'fc_vertex_frames', 'fc_logmap', 'fc_logmap_workspace_bytes', 'fc_logmap_ball_lds_vertices'}
    assert names <= declared and names <= set(_lib.SIGNATURES) and 'fc_logmap.hip' in build.SOURCES and 'fc_geodesic_relax.hpp' in build.HEADERS
