"""The device's edge graph with unfolded diagonals (fieldconv_amd.geodesic.mesh_edge_graph(..., diagonals=True),
csrc/fc_mesh_graph.hip) against the numpy restatement tests/_diagonal_graph_ref.py, bit for bit; and every consumer run with
diagonals=True against the existing restatements (tests/_geodesic_ref.py, _geodesic_sampling_ref.py, _logmap_ref.py) fed the
restated enriched graph: they take any (ptr, nbr, length), so everything carries over exactly; the log map's values by
test_gpu_logmap.py's criterion (4 x the float32 restatement's own error against float64 on the same tree)."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _diagonal_graph_ref as dref
import _geodesic_ref as gref
import _geodesic_sampling_ref as sref
import _logmap_ref as lref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else (t.view(torch.int32) if t.dtype == torch.float32 else t)


# every mesh and reference is computed once and shared (the tests only read them)
@functools.lru_cache(maxsize=None)
def mesh(name):
    if name == 'ico':
        return lref.icosphere(2)                  # 162 vertices, closed
    if name == 'grid':
        return lref.jittered_grid(9, 7)           # 63 vertices: obtuse triangles and a boundary
    if name == 'two':
        return lref.two_components()              # two components, a vertex in no face, a zero-length side
    if name == 'joined':
        return dref.joined()[:2]                  # the hand-made meshes of the host test as one mesh
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def graph(name):
    return dref.edge_graph(*mesh(name))


EPSILON = {'ico': 0.7, 'grid': 0.3}
BOUND = {'ico': 0.85, 'grid': 0.45}


@functools.lru_cache(maxsize=None)
def samples(name):
    """32 geodesic FPS samples of the restated enriched graph from vertex 0, in selection order, and the final field"""
    return sref.fps(*graph(name), 32, 0)


def assert_graph(got, want):
    ptr, nbr, length = got
    assert ptr.dtype == torch.int32 and nbr.dtype == torch.int32 and length.dtype == torch.float32
    assert np.array_equal(N_(ptr), want[0]) and np.array_equal(N_(nbr), want[1])
    assert np.array_equal(N_(length).view(np.uint32), want[2].view(np.uint32))


# ------------------------------------------------------------------ 1. the graph
@pytest.mark.parametrize('name', ['ico', 'grid', 'two', 'joined'])
def test_graph_equals_the_restatement(dev, name):
    from fieldconv_amd.geodesic import _graph_on, mesh_edge_graph
    pos, face = mesh(name)
    want, side = graph(name), gref.edge_graph(pos, face)
    got = mesh_edge_graph(T(pos, dev), T(face, dev), diagonals=True)
    assert all(t.device == dev for t in got)
    assert_graph(got, want)
    assert len(want[1]) > len(side[1])            # (every one of these meshes gains diagonals)
    _graph_on(got, pos.shape[0], dev, 'test')      # a valid graph= for every consumer
    again = mesh_edge_graph(T(pos, dev), T(face, dev), diagonals=True)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again))
    # host tensors in, host tensors out
    cpu = mesh_edge_graph(torch.from_numpy(pos), torch.from_numpy(face), diagonals=True)
    assert all(not a.is_cuda and torch.equal(bits(a), bits(b).cpu()) for a, b in zip(cpu, got))


def test_batch_graph_is_the_meshes_graphs_offset_and_concatenated(dev):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.geodesic import mesh_edge_graph
    names = ['grid', 'ico']
    batch = MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(mesh(n)[0]), face=torch.from_numpy(mesh(n)[1])) for n in names]).to(dev)
    assert batch.pos_ptr.tolist() == [0, 63, 63 + 162]
    got = mesh_edge_graph(batch.pos, batch.face, diagonals=True)
    parts = [graph(n) for n in names]
    ptr = np.concatenate(([0], np.cumsum(np.concatenate([np.diff(p[0]) for p in parts]))))
    nbr = np.concatenate([p[1] + o for p, o in zip(parts, (0, 63))])
    assert_graph(got, (ptr, nbr, np.concatenate([p[2] for p in parts])))
    single = [mesh_edge_graph(T(mesh(n)[0], dev), T(mesh(n)[1], dev), diagonals=True) for n in names]
    assert torch.equal(got[1], torch.cat((single[0][1], single[1][1] + 63)))
    assert torch.equal(bits(got[2]), bits(torch.cat((single[0][2], single[1][2]))))


@pytest.mark.parametrize('name', ['ico', 'grid', 'two', 'joined'])
def test_without_diagonals_nothing_changes(dev, name):
    """diagonals=False (and the default) return what the construction before the keyword gave: the torch recipe, recomputed
    here, and fc_mesh_edge_lengths on its slots"""
    import ctypes
    from fieldconv_amd import _lib
    from fieldconv_amd.geodesic import mesh_edge_graph
    pos, face = mesh(name)
    p, f = T(pos, dev), T(face, dev)
    V = int(p.shape[0])
    a = torch.cat((f[0], f[1], f[2], f[1], f[2], f[0]))
    b = torch.cat((f[1], f[2], f[0], f[0], f[1], f[2]))
    key = torch.unique(a * V + b)
    src, nbr = key // V, key % V
    keep = src != nbr
    src, nbr = src[keep].contiguous(), nbr[keep]
    ptr = torch.searchsorted(src, torch.arange(V + 1, device=dev)).to(torch.int32)
    src, nbr = src.to(torch.int32), nbr.to(torch.int32).contiguous()
    E = int(nbr.numel())
    length = torch.empty(E, dtype=torch.float32, device=dev)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    _lib.check(_lib.load().fc_mesh_edge_lengths(vp(p), vp(src), vp(nbr), V, E, vp(length),
                                                ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), 'fc_mesh_edge_lengths')
    for got in (mesh_edge_graph(p, f), mesh_edge_graph(p, f, diagonals=False)):
        assert got[0].dtype == torch.int32 and got[1].dtype == torch.int32
        assert torch.equal(got[0], ptr) and torch.equal(got[1], nbr) and torch.equal(bits(got[2]), bits(length))
    assert_graph((ptr, nbr, length), gref.edge_graph(pos, face))


# ------------------------------------------------------------------ 2. the consumers over the enriched graph
@pytest.mark.parametrize('name', ['ico', 'grid'])
def test_distances_labels_and_weights(dev, name):
    from fieldconv_amd.geodesic import geodesic_distances, geodesic_error, nearest_sample, sample_weights, samples_to_nearest
    pos, face = mesh(name)
    p, f = T(pos, dev), T(face, dev)
    V = pos.shape[0]
    g = graph(name)
    sources = gref.spread(V, 9, seed=3)
    rows = geodesic_distances(p, f, T(sources, dev), diagonals=True)
    want = np.stack([gref.dijkstra32(*g, [s]) for s in sources])
    assert np.array_equal(N_(rows).view(np.uint32), want.view(np.uint32))
    side = np.stack([gref.dijkstra32(*gref.edge_graph(pos, face), [s]) for s in sources])
    assert (want <= side).all() and (want < side).any()          # a richer graph: never longer, somewhere shorter

    label, dist = nearest_sample(p, f, T(sources, dev), diagonals=True)
    d = gref.dijkstra32(*g, sources)
    want_label = gref.tight_labels(*g, d, sources)
    assert np.array_equal(N_(dist).view(np.uint32), d.view(np.uint32)) and np.array_equal(N_(label), want_label)
    assert torch.equal(samples_to_nearest(p, f, T(sources, dev), diagonals=True), label)
    w = sample_weights(p, f, T(sources, dev), diagonals=True)
    assert np.array_equal(N_(w).view(np.uint32), gref.sample_weights(pos, face, want_label, 9).view(np.uint32))

    # the error of a prediction is an entry of a distance row, divided in float32 by sqrt(area)
    pred, target = T(gref.spread(V, 20, seed=4), dev), T(sources[np.arange(20) % 9], dev)
    err = geodesic_error(p, f, pred, target, normalize=False, diagonals=True)
    assert np.array_equal(N_(err).view(np.uint32), want[np.arange(20) % 9, N_(pred)].view(np.uint32))


@pytest.mark.parametrize('name', ['ico', 'grid'])
def test_sampling_and_ball_edges(dev, name):
    from fieldconv_amd.geodesic_sampling import (geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched,
                                                 geodesic_radius_edges)
    pos, face = mesh(name)
    p, f = T(pos, dev), T(face, dev)
    want_idx, want_field = samples(name)
    idx, field = geodesic_farthest_point_sample(p, f, 32, 0, return_dist=True, diagonals=True)
    assert np.array_equal(N_(idx), want_idx) and np.array_equal(N_(field).view(np.uint32), want_field.view(np.uint32))
    one = geodesic_farthest_point_sample_batched(p, f, torch.tensor([0, pos.shape[0]]), 32, 0, diagonals=True)
    assert torch.equal(one, idx)
    chosen = np.sort(want_idx)
    edges, dist = geodesic_radius_edges(p, f, T(chosen, dev), EPSILON[name], return_dist=True, diagonals=True)
    want_edges, want_dist = sref.ball_edges(*graph(name), chosen, EPSILON[name])
    assert np.array_equal(N_(edges), want_edges) and np.array_equal(N_(dist).view(np.uint32), want_dist.view(np.uint32))
    side_edges, _ = sref.mesh_ball_edges(pos, face, chosen, EPSILON[name])
    assert len(want_edges) >= len(side_edges)          # no distance grows: the same ball holds at least the same samples


@functools.lru_cache(maxsize=None)
def logmap_case(name):
    """rows: every pair of samples within twice the bound of each other, so some are reached and some take the fallback -- but not
    the near-antipodal pairs of the sphere, whose chord has next to no tangential part: its direction, and with it the float32
    restatement's own error, would be of the size of L itself and the gate would check nothing"""
    pos, face = mesh(name)
    chosen = np.sort(samples(name)[0])
    rows, _ = sref.ball_edges(*graph(name), chosen, 2 * BOUND[name])
    return dref.GraphCase(pos, face, chosen, rows, BOUND[name])


@functools.lru_cache(maxsize=None)
def logmap_result(name):
    from fieldconv_amd.logmap import log_map_transport
    c, dev = logmap_case(name), torch.device('cuda:0')
    return log_map_transport(T(c.pos, dev), T(c.face, dev), T(c.sample_idx, dev), T(c.edges, dev), c.bound, return_reached=True,
                             return_tree=True, diagonals=True)


@pytest.mark.parametrize('name', ['ico', 'grid'])
def test_log_map_trees_and_values(dev, name):
    c = logmap_case(name)
    mag, ang, xp, reached, pred, hops = logmap_result(name)
    assert np.array_equal(N_(hops), c.h) and np.array_equal(N_(pred), c.pred)
    assert np.array_equal(N_(reached), c.reached) and c.reached.any() and not c.reached.all()          # some rows take the fallback
    used = {(int(c.pred[q, v]), int(v)) for q in range(32) for v in np.nonzero(c.pred[q] >= 0)[0]}
    assert used - set(dref.pairs_of(*gref.edge_graph(c.pos, c.face)))                                  # the trees do run over diagonals
    (L32, X32), (L64, X64) = c.values(np.float32), c.values(np.float64)
    rebuilt = lambda m, a: m.astype(np.float64) * np.exp(1j * a.astype(np.float64))
    L64c, X64c = lref.as_complex(L64), lref.as_complex(X64)
    own_L = float(np.abs(rebuilt(*lref.polar(L32)) - L64c).max())
    own_X = float(np.abs(lref.as_complex(X32) - X64c).max())
    gate_L, gate_X = max(4 * own_L, 1e-6 * float(np.abs(L64c).max())), max(4 * own_X, 1e-6)
    err_L = float(np.abs(rebuilt(N_(mag), N_(ang)) - L64c).max())
    err_X = float(np.abs(N_(xp).astype(np.complex128) - X64c).max())
    print(f'\n{name}: device against float64 L {err_L:.3e} X {err_X:.3e}; float32 restatement against float64 L {own_L:.3e} X {own_X:.3e}; '
          f'gates {gate_L:.3e} {gate_X:.3e}')
    assert err_L <= gate_L and err_X <= gate_X


@pytest.mark.parametrize('name', ['ico', 'grid'])
def test_transforms_with_diagonals_reach_every_row(dev, name):
    from fieldconv_amd.geodesic import mesh_edge_graph, sample_weights
    from fieldconv_amd.logmap import log_map_transport
    from fieldconv_amd.transforms import ComputeLogXPort, GeodesicSupportGraph, SampleWeights
    pos, face = mesh(name)
    p, f = T(pos, dev), T(face, dev)
    eps = EPSILON[name]
    data = GeodesicSupportGraph(epsilon=eps, sample_n=32, random_start=False, diagonals=True)(SimpleNamespace(pos=p, face=f))
    chosen = np.sort(samples(name)[0])
    assert np.array_equal(N_(data.sample_idx), chosen)
    assert np.array_equal(N_(data.supp_edges), sref.ball_edges(*graph(name), chosen, eps)[0])
    data = ComputeLogXPort(eps, diagonals=True)(data)
    mag, ang, xp, reached = log_map_transport(p, f, data.sample_idx, data.supp_edges, eps, return_reached=True, diagonals=True)
    assert reached.dtype == torch.bool and bool(reached.all())
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip((data.logMag, data.logAng, data.xp), (mag, ang, xp)))
    w = sample_weights(p, f, data.sample_idx, diagonals=True)
    assert torch.equal(bits(data.w), bits(w))
    assert torch.equal(bits(SampleWeights(diagonals=True)(SimpleNamespace(pos=p, face=f, sample_idx=data.sample_idx)).w), bits(w))
    # a graph built with diagonals is a graph= like any other
    rich = mesh_edge_graph(p, f, diagonals=True)
    via = log_map_transport(p, f, data.sample_idx, data.supp_edges, eps, graph=rich)
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(via, (mag, ang, xp)))


# ------------------------------------------------------------------ 3. arguments
def test_graph_together_with_diagonals_raises_and_host_tensors_work(dev):
    from fieldconv_amd import geodesic as G
    from fieldconv_amd import geodesic_sampling as GS
    from fieldconv_amd.logmap import log_map_transport
    from fieldconv_amd.transforms import ComputeLogXPort, GeodesicSupportGraph, SampleWeights
    pos, face = mesh('grid')
    p, f = torch.from_numpy(pos), torch.from_numpy(face)          # on the host
    rich = G.mesh_edge_graph(p, f, diagonals=True)
    idx = torch.tensor([0, 20, 41], dtype=torch.int64)
    pairs = torch.from_numpy(lref.all_pairs(3))
    ptr = torch.tensor([0, 63])
    both = [
        lambda: G.geodesic_distances(p, f, idx, graph=rich, diagonals=True),
        lambda: G.nearest_sample(p, f, idx, graph=rich, diagonals=True),
        lambda: G.sample_weights(p, f, idx, graph=rich, diagonals=True),
        lambda: G.geodesic_error(p, f, idx, idx, graph=rich, diagonals=True),
        lambda: GS.geodesic_farthest_point_sample(p, f, 4, graph=rich, diagonals=True),
        lambda: GS.geodesic_farthest_point_sample_batched(p, f, ptr, 4, graph=rich, diagonals=True),
        lambda: GS.geodesic_radius_edges(p, f, idx, 0.3, graph=rich, diagonals=True),
        lambda: log_map_transport(p, f, idx, pairs, 0.3, graph=rich, diagonals=True),
        lambda: SampleWeights(diagonals=True, graph=rich),
        lambda: G.mesh_edge_graph(p, f, diagonals=1),                       # not a bool
        lambda: G.nearest_sample(p, f, idx, diagonals='yes'),
        lambda: GeodesicSupportGraph(0.3, diagonals=None),
        lambda: ComputeLogXPort(0.3, diagonals=0),
        lambda: G.mesh_edge_graph(p.double(), f, diagonals=True),           # the mesh is checked as before
        lambda: G.mesh_edge_graph(p, f.t().contiguous(), diagonals=True),
    ]
    for i, call in enumerate(both):
        with pytest.raises(ValueError):
            call()
            pytest.fail(f'case {i} did not raise')
    # host tensors in, host tensors out, the device's bits; graph= alone gives what diagonals=True gives
    pd, fd = p.to(dev), f.to(dev)
    for fn, args in ((G.geodesic_distances, (idx,)), (G.nearest_sample, (idx,)), (G.sample_weights, (idx,)),
                     (GS.geodesic_farthest_point_sample, (8,)), (GS.geodesic_radius_edges, (idx, 0.3)), (log_map_transport, (idx, pairs, 0.3))):
        host = fn(p, f, *args, diagonals=True)
        device = fn(pd, fd, *[a.to(dev) if torch.is_tensor(a) else a for a in args], diagonals=True)
        via = fn(p, f, *args, graph=rich)
        host, device, via = [x if isinstance(x, tuple) else (x,) for x in (host, device, via)]
        for h, d, v in zip(host, device, via):
            assert not h.is_cuda and d.device == dev and torch.equal(bits(h), bits(d).cpu()) and torch.equal(bits(h), bits(v))
