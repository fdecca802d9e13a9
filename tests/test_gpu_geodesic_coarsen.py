"""Geodesic coarsening on the device -- farthest-point sampling among candidates (fc_geodesic_fps_among), balls for a list of
queries (fc_geodesic_ball_count_at / _fill_at) and transforms.CoarsenSamples(sampling='geodesic') -- against the numpy
restatement tests/_geodesic_coarsen_ref.py: indices equal, distances bit for bit; everything is a function of least fixpoints,
so there is nothing to tolerate.  Shapes sit where the kernels can go wrong: exact ties, every candidate taken, +inf candidates,
an irregular surface, sizes around the 1024 threads of the workgroup, one vertex above the LDS capacity (the global-memory
instantiation), batches that mix both instantiations, and a request for more samples than there are candidates."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _geodesic_coarsen_ref as cref
import _geodesic_ref as gref
import _geodesic_sampling_ref as sref

pytestmark = pytest.mark.gpu

CAP = 20000


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def same_bits(got, want):
    got = N_(got)
    return got.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


MESHES = {
    'lattice': lambda: gref.lattice(23, 17),
    'small_lattice': lambda: gref.lattice(6, 5),
    'surface': lambda: gref.surface(1500, seed=3),
    'surface300': lambda: gref.surface(300, seed=1),
    'odd': sref.odd_mesh,
    'v1023': lambda: gref.lattice(33, 31), 'v1024': lambda: gref.lattice(32, 32), 'v1025': lambda: gref.lattice(25, 41),
    'cap+1': lambda: gref.lattice(6667, 3),
    'l79': lambda: gref.lattice(7, 9), 'l54': lambda: gref.lattice(5, 4),
    'folded': lambda: cref.folded_strip(41, 9, 0.125, 0.05),
}


# every mesh, graph and reference is computed once and shared (the tests only read them)
@functools.lru_cache(maxsize=None)
def mesh(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def graph(name):
    return gref.edge_graph(*mesh(name))


def every(name, step):
    return np.arange(0, mesh(name)[0].shape[0], step, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def _among(name, cand_bytes, n_samples, start):
    return cref.fps_among(*graph(name), np.frombuffer(cand_bytes, dtype=np.int64), n_samples, start)


def among_case(name, cand, n_samples, start):
    return _among(name, np.ascontiguousarray(cand, dtype=np.int64).tobytes(), n_samples, int(start))


def check_among(dev, name, cand, n_samples, start):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample
    pos, face = mesh(name)
    want_idx, want_d = among_case(name, cand, n_samples, start)
    idx, dist, sweeps = geodesic_farthest_point_sample(T(pos, dev), T(face, dev), n_samples, int(start), return_dist=True, return_sweeps=True,
                                                       candidates=T(cand, dev))
    assert idx.dtype == torch.int64 and idx.device == dev and dist.device == dev
    assert np.array_equal(N_(idx), want_idx)
    assert same_bits(dist, want_d)
    assert int(sweeps) >= n_samples
    return idx, dist


# ------------------------------------------------------------------ sampling among candidates
def test_among_lattice_with_exact_ties(dev):
    cand = every('lattice', 3)
    tied = []

    def count_ties(k, taken, field, free):
        tied.append(len(free) > 0 and int((field[free] == field[free].max()).sum()) > 1)
    cref.fps_among(*graph('lattice'), cand, 32, cand[2], each_round=count_ties)
    assert sum(tied) >= 4, 'the lattice must tie for the next choice in several rounds'
    idx, _ = check_among(dev, 'lattice', cand, 32, cand[2])
    assert set(N_(idx).tolist()) <= set(cand.tolist())


def test_among_takes_every_candidate_exactly_once(dev):
    cand = np.array([0, 2, 5, 7, 11, 12, 16, 19, 23, 26, 29], dtype=np.int64)
    idx, _ = check_among(dev, 'small_lattice', cand, 11, 11)
    assert sorted(N_(idx).tolist()) == cand.tolist()


def test_among_unreachable_candidates_come_first(dev):
    """vertex 46 is in no face, 33 in the second component, 47 the zero-length copy of 14: +inf first, lowest number first"""
    cand = np.array([2, 7, 14, 20, 29, 33, 46, 47], dtype=np.int64)
    idx, _ = check_among(dev, 'odd', cand, 8, 7)
    got = N_(idx).tolist()
    assert got[:3] == [7, 33, 46] and sorted(got) == cand.tolist()


def test_among_irregular_surface(dev):
    cand = np.sort(gref.spread(1500, 400))
    check_among(dev, 'surface', cand, 48, cand[0])


def test_among_all_vertices_is_the_unrestricted_sampling(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample
    for name in ('surface', 'odd'):
        pos, face = mesh(name)
        p, f = T(pos, dev), T(face, dev)
        want = geodesic_farthest_point_sample(p, f, 40, 3, return_dist=True)
        got = geodesic_farthest_point_sample(p, f, 40, 3, return_dist=True, candidates=torch.arange(pos.shape[0], device=dev))
        assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))


@pytest.mark.parametrize('name', ['v1023', 'v1024', 'v1025'])
def test_among_workgroup_remainder(dev, name):
    check_among(dev, name, every(name, 5), 8, 0)


def test_among_above_the_lds_capacity(dev):
    """one vertex more than the LDS capacity: the global-memory instantiation reads the mask too"""
    assert mesh('cap+1')[0].shape[0] == CAP + 1
    check_among(dev, 'cap+1', every('cap+1', 7), 4, 0)


def _batch(names, cands):
    pos, face, pos_ptr = gref.union([mesh(n) for n in names])
    union_cand = np.concatenate([c + o for c, o in zip(cands, pos_ptr[:-1])])
    cand_ptr = np.cumsum([0] + [len(c) for c in cands]).astype(np.int64)
    return pos, face, pos_ptr, union_cand, cand_ptr


def check_among_batch(dev, names, cands, counts, starts):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched
    pos, face, pos_ptr, union_cand, cand_ptr = _batch(names, cands)
    idx, dist = geodesic_farthest_point_sample_batched(T(pos, dev), T(face, dev), T(pos_ptr, dev), counts, starts, return_dist=True,
                                                       candidates=T(union_cand, dev), candidates_ptr=T(cand_ptr, dev))
    assert idx.shape == (sum(counts),)
    out = np.cumsum([0] + counts)
    for b, name in enumerate(names):
        want_idx, want_d = among_case(name, cands[b], counts[b], starts[b])
        p, f = mesh(name)
        one = geodesic_farthest_point_sample(T(p, dev), T(f, dev), counts[b], starts[b], candidates=T(cands[b], dev))
        assert np.array_equal(N_(one), want_idx)
        assert np.array_equal(N_(idx[out[b]:out[b + 1]]), want_idx)          # local to the mesh, in selection order
        assert same_bits(dist[pos_ptr[b]:pos_ptr[b + 1]], want_d)


def test_among_batch_equals_single_calls(dev):
    names = ['l79', 'surface300', 'l54']
    cands = [every('l79', 2), np.sort(gref.spread(300, 90, seed=2)), every('l54', 3)]
    check_among_batch(dev, names, cands, [11, 9, 5], [int(cands[0][3]), int(cands[1][0]), int(cands[2][1])])


def test_among_batch_mixes_both_instantiations(dev):
    check_among_batch(dev, ['l54', 'cap+1'], [every('l54', 3), every('cap+1', 7)], [4, 4], [3, 0])


def test_among_more_samples_than_candidates_through_the_abi(dev):
    """the kernel's guard, which the functional layer never reaches: 3 candidates, 5 rounds asked -> FC_OK, the three taken, -1
    in the remaining slots, dist the field of the three, and nothing written around idx"""
    from fieldconv_amd import _lib
    from fieldconv_amd._launch import ptr as _ptr, stream as _stream
    from fieldconv_amd.geodesic import mesh_edge_graph
    pos, face = mesh('lattice')
    V = pos.shape[0]
    cand = np.array([5, 200, 390], dtype=np.int64)
    want_idx, want_d = among_case('lattice', cand, 3, 200)
    lib = _lib.load()
    with torch.cuda.device(dev):
        ptr, nbr, length = mesh_edge_graph(T(pos, dev), T(face, dev))
        mask = torch.zeros(V, dtype=torch.uint8, device=dev)
        mask[T(cand, dev)] = 1
        tables = torch.tensor([[5], [200], [0]], dtype=torch.int64, device=dev)
        buf = torch.full((13,), -7777, dtype=torch.int64, device=dev)
        idx = buf[4:9]
        dist = torch.full((V,), -1.0, dtype=torch.float32, device=dev)
        status = lib.fc_geodesic_fps_among(_ptr(ptr), _ptr(nbr), _ptr(length), V, int(nbr.numel()), None, 1, V, _ptr(mask), _ptr(tables[0]),
                                           _ptr(tables[1]), _ptr(tables[2]), 5, idx.data_ptr(), _ptr(dist), None, None, 0, _stream())
        torch.cuda.synchronize(dev)
    assert status == 0
    got = N_(buf)
    assert np.array_equal(got[4:7], want_idx) and got[7:9].tolist() == [-1, -1]
    assert (got[:4] == -7777).all() and (got[9:] == -7777).all()
    assert same_bits(dist, want_d)


# ------------------------------------------------------------------ balls for chosen queries
@functools.lru_cache(maxsize=None)
def ball_case(name, epsilon, k=512):
    """the 64 sorted samples of the mesh's unrestricted sampling and all their ball edges"""
    pos, face = mesh(name)
    samples = np.sort(sref.fps(*graph(name), 64, 5)[0])
    return (pos, face, samples) + sref.ball_edges(*graph(name), samples, epsilon, k)


def check_ball_at(dev, name, epsilon, queries, k=512):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face, samples, all_e, all_d = ball_case(name, epsilon, k)
    want_e, want_d = cref.ball_edges_at(all_e, all_d, queries)
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(samples, dev), epsilon, k, return_dist=True, queries=T(queries, dev))
    assert edges.dtype == torch.int64 and edges.device == dev and tuple(edges.shape) == want_e.shape
    assert np.array_equal(N_(edges), want_e)
    assert same_bits(dist, want_d)
    assert torch.equal(geodesic_radius_edges(T(pos, dev), T(face, dev), T(samples, dev), epsilon, k, queries=T(queries, dev)), edges)
    return edges, dist


THIRD = np.arange(0, 64, 3, dtype=np.int64)


def test_ball_at_lattice_excludes_distances_equal_to_epsilon(dev):
    """epsilon = 4 h is exactly representable and sample pairs lie at exactly that distance: the comparison is strict"""
    pos, face, samples, all_e, _ = ball_case('lattice', 0.5)
    rows = gref.rows(pos, face, samples[THIRD])[:, samples]
    assert (rows == np.float32(0.5)).any()
    edges, _ = check_ball_at(dev, 'lattice', 0.5, THIRD)
    assert len(edges) == (rows < np.float32(0.5)).sum() and 0 < len(edges) < len(all_e)


def test_ball_at_cap_keeps_the_nearest(dev):
    _, _, _, all_e, _ = ball_case('lattice', 0.5)
    assert (np.bincount(all_e[:, 0], minlength=64)[THIRD] > 4).any(), 'the cap must bite on a listed query'
    edges, _ = check_ball_at(dev, 'lattice', 0.5, THIRD, 4)
    assert int(torch.bincount(edges[:, 0], minlength=64).max()) == 4


def test_ball_at_every_query_is_the_plain_call(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face, samples, _, _ = ball_case('lattice', 0.5)
    p, f, s = T(pos, dev), T(face, dev), T(samples, dev)
    want = geodesic_radius_edges(p, f, s, 0.5, return_dist=True)
    got = geodesic_radius_edges(p, f, s, 0.5, return_dist=True, queries=torch.arange(64, device=dev))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
    check_ball_at(dev, 'lattice', 0.5, np.arange(64, dtype=np.int64))


def test_ball_at_no_queries(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face, samples, _, _ = ball_case('lattice', 0.5)
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(samples, dev), 0.5, return_dist=True,
                                        queries=torch.zeros(0, dtype=torch.int64, device=dev))
    assert tuple(edges.shape) == (0, 2) and edges.dtype == torch.int64 and edges.device == dev
    assert tuple(dist.shape) == (0,) and dist.dtype == torch.float32 and dist.device == dev


def test_ball_at_batch_with_queries_across_the_meshes(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    names = ['l79', 'surface300', 'l54']
    local = [every('l79', 5), np.sort(gref.spread(300, 24, seed=4)), every('l54', 2)]
    eps = 0.3
    pos, face, pos_ptr, union_idx, sample_ptr = _batch(names, local)
    want_e, want_d = [], []
    for b, name in enumerate(names):
        e, d = sref.ball_edges(*graph(name), local[b], eps)
        want_e.append(e + sample_ptr[b])
        want_d.append(d)
    want_e, want_d = np.concatenate(want_e), np.concatenate(want_d)
    S = len(union_idx)
    queries = np.array([0, 5, 12, 13, 20, 36, 37, S - 4, S - 1], dtype=np.int64)
    assert [int(np.searchsorted(sample_ptr, q, side='right')) - 1 for q in queries].count(1) >= 3 and queries[-1] >= sample_ptr[2]
    want_e, want_d = cref.ball_edges_at(want_e, want_d, queries)
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(union_idx, dev), eps, pos_ptr=T(pos_ptr, dev), sample_ptr=T(sample_ptr, dev),
                                        return_dist=True, queries=T(queries, dev))
    assert np.array_equal(N_(edges), want_e) and same_bits(dist, want_d)


# eight samples of the strip above the LDS capacity, some within reach of each other and some at exactly 3 h
CLUSTERED = np.array([0, 4, 9, 3000, 3003, 10000, 10001, 20000], dtype=np.int64)


def test_ball_at_above_the_lds_capacity(dev):
    """three workspace slots for the queries 1, 4 and 7 = S - 1: a slot belongs to the list slot, not to the query"""
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face = mesh('cap+1')
    queries = np.array([1, 4, 7], dtype=np.int64)
    want_e, want_d = cref.ball_edges_at(*sref.ball_edges(*graph('cap+1'), CLUSTERED, 0.375, bounded=True), queries)
    assert len(want_e) > 3 and set(want_e[:, 0].tolist()) == {1, 4, 7}
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(CLUSTERED, dev), 0.375, return_dist=True, queries=T(queries, dev))
    assert np.array_equal(N_(edges), want_e) and same_bits(dist, want_d)


# ------------------------------------------------------------------ the transform
FINE_EPS, COARSE_EPS = 0.15, 0.3


def fine_level(dev, name, epsilon, sample_n, diagonals=False, sample_idx=None):
    from fieldconv_amd.transforms import ComputeLogXPort, GeodesicSupportGraph
    pos, face = mesh(name)
    data = SimpleNamespace(pos=T(pos, dev), face=T(face, dev))
    if sample_idx is not None:
        data.sample_idx = T(sample_idx, dev)
    data = GeodesicSupportGraph(epsilon, sample_n=sample_n, random_start=False, diagonals=diagonals)(data)
    return ComputeLogXPort(epsilon, diagonals=diagonals)(data)


def test_transform_samples_geodesically_among_the_fine_samples(dev):
    from fieldconv_amd.nn import TangentPool
    from fieldconv_amd.transforms import CoarsenSamples, FCPrecomp
    fine = fine_level(dev, 'surface', FINE_EPS, 256)
    coarse = CoarsenSamples(64, COARSE_EPS, sampling='geodesic')(fine)
    fine_idx = N_(fine.sample_idx)
    want = cref.coarsen_geodesic(*graph('surface'), fine_idx, 64)
    got = N_(coarse.coarse)
    assert np.array_equal(got, want) and (np.diff(got) > 0).all() and got.shape == (64,)
    assert torch.equal(coarse.sample_idx, fine.sample_idx[coarse.coarse])
    assert not np.array_equal(got, N_(CoarsenSamples(64, COARSE_EPS)(fine).coarse))          # (the default stays Euclidean)
    # an explicit coarse overrides the rule; more than there are: every fine sample
    chosen = torch.arange(0, 256, 4, device=dev)
    assert torch.equal(CoarsenSamples(64, COARSE_EPS, sampling='geodesic', coarse=chosen)(fine).coarse, chosen)
    # the level is a level: FCPrecomp and the pooling take it
    edges, sten = FCPrecomp(2, 6, COARSE_EPS)(coarse)[:2]
    assert edges.shape[0] > 64 and int(edges.max()) < 64
    x = torch.randn(256, 4, dtype=torch.complex64).to(dev)
    y = TangentPool()(x, coarse)
    assert tuple(y.shape) == (64, 4) and bool(torch.isfinite(torch.view_as_real(y)).all())


def test_transform_with_diagonals_samples_on_the_diagonal_graph(dev):
    import _diagonal_graph_ref as dref
    from fieldconv_amd.transforms import CoarsenSamples
    fine = fine_level(dev, 'surface300', 0.3, 96, diagonals=True)
    coarse = CoarsenSamples(24, 0.6, diagonals=True, sampling='geodesic', interpolate_k=3)(fine)
    want = cref.coarsen_geodesic(*dref.edge_graph(*mesh('surface300')), N_(fine.sample_idx), 24)
    assert np.array_equal(N_(coarse.coarse), want)
    assert coarse.interp.n_out == 96 and coarse.interp.n_in == 24
    all_of_them = CoarsenSamples(500, 0.6, diagonals=True, sampling='geodesic')(fine)
    assert torch.equal(all_of_them.coarse, torch.arange(96, device=dev))


def test_transform_batch_equals_single_calls(dev):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    names = ['l79', 'surface300', 'l54']

    def chain(data):
        data = GeodesicSupportGraph(0.3, sample_n=40, random_start=False)(data)
        data = ComputeLogXPort(0.3)(data)
        return data, CoarsenSamples(8, 0.6, sampling='geodesic')(data)
    singles = [chain(SimpleNamespace(pos=T(mesh(n)[0], dev), face=T(mesh(n)[1], dev))) for n in names]
    fine, coarse = chain(MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(mesh(n)[0]), face=torch.from_numpy(mesh(n)[1]))
                                              for n in names]).to(dev))
    assert fine.ptr.tolist() == [0, 40, 80, 100] and coarse.ptr.tolist() == [0, 8, 16, 24]
    assert torch.equal(coarse.coarse, torch.cat([c.coarse + o for (_, c), o in zip(singles, (0, 40, 80))]))
    assert torch.equal(coarse.sample_idx, torch.cat([c.sample_idx + o for (_, c), o in zip(singles, (0, 63, 363))]))
    for (f, c), name in zip(singles, names):
        assert np.array_equal(N_(c.coarse), cref.coarsen_geodesic(*graph(name), N_(f.sample_idx), 8))


def test_transform_covers_the_folded_strip_as_the_restatement_says(dev):
    """the host test's two covering radii (tests/test_geodesic_coarsen_host.py), from the device: every second vertex of the
    folded strip, 16 coarse samples by either rule"""
    from fieldconv_amd.geodesic import nearest_sample
    from fieldconv_amd.transforms import CoarsenSamples
    pos, face = mesh('folded')
    fine_idx = every('folded', 2)
    fine = fine_level(dev, 'folded', 0.4, None, sample_idx=fine_idx)
    radius = {}
    for rule in ('geodesic', 'euclidean'):
        coarse = CoarsenSamples(16, 1.5, sampling=rule)(fine)
        field = nearest_sample(fine.pos, fine.face, coarse.sample_idx)[1]
        radius[rule] = float(field[fine.sample_idx].max())
    want_geo = cref.covering_radius(*graph('folded'), fine_idx, fine_idx[cref.coarsen_geodesic(*graph('folded'), fine_idx, 16)])
    want_euc = cref.covering_radius(*graph('folded'), fine_idx, fine_idx[cref.euclidean_fps(pos[fine_idx], 16, 0)])
    print(f'folded strip on the device: covering radius geodesic {radius["geodesic"]:.4f}, Euclidean {radius["euclidean"]:.4f}')
    assert radius['geodesic'] == want_geo and radius['euclidean'] == want_euc and radius['geodesic'] < radius['euclidean']
