"""Mesh geodesics on the device (fieldconv_amd.geodesic, csrc/fc_geodesic.hip) against the numpy float32 restatement
tests/_geodesic_ref.py: distances bit for bit, labels exactly -- the fixpoint is unique whatever the order of the
relaxations, so there is nothing to tolerate.  Shapes sit where the solver can go wrong: exact ties (a binary lattice),
an irregular surface, unreachable and faceless vertices, duplicate sources and zero-length edges, the LDS capacity and
one vertex more (the global-memory instantiation), sizes around the 1024 threads of the workgroup, and mini-batches that mix
both instantiations."""
import functools

import numpy as np
import pytest
import torch

import _geodesic_ref as gref

pytestmark = pytest.mark.gpu


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


# every reference is computed once and shared (the tests only read it)
@functools.lru_cache(maxsize=None)
def lattice_case(nx, ny, n_sources):
    pos, face = gref.lattice(nx, ny)
    sources = gref.spread(nx * ny, n_sources, seed=nx)
    return (pos, face, sources) + gref.nearest(pos, face, sources)


@functools.lru_cache(maxsize=None)
def surface_case():
    pos, face = gref.surface(400, seed=1)
    sources = gref.spread(400, 9)
    return (pos, face, sources) + gref.nearest(pos, face, sources)


def check_nearest(dev, pos, face, sources, want_label, want_dist, **kw):
    from fieldconv_amd.geodesic import nearest_sample
    label, dist, sweeps = nearest_sample(T(pos, dev), T(face, dev), T(sources, dev), return_sweeps=True, **kw)
    assert label.dtype == torch.int64 and label.device == dev and dist.device == dev
    assert same_bits(dist, want_dist)
    assert np.array_equal(N_(label), want_label)
    assert (N_(sweeps) >= 1).all()
    return N_(sweeps)


# ------------------------------------------------------------------ the contract, shape by shape
def test_lattice_with_exact_ties(dev):
    pos, face, sources, label, dist = lattice_case(13, 13, 9)
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert gref.tied_vertices(ptr, nbr, length, dist, label), 'the lattice must hold a vertex whose tight predecessors disagree'
    check_nearest(dev, pos, face, sources, label, dist)


def test_edge_graph_matches_the_restatement(dev):
    from fieldconv_amd.geodesic import mesh_edge_graph
    pos, face, *_ = surface_case()
    ptr, nbr, length = mesh_edge_graph(T(pos, dev), T(face, dev))
    w_ptr, w_nbr, w_len = gref.edge_graph(pos, face)
    assert ptr.dtype == torch.int32 and nbr.dtype == torch.int32
    assert np.array_equal(N_(ptr), w_ptr) and np.array_equal(N_(nbr), w_nbr) and same_bits(length, w_len)


def test_irregular_surface_nearest_and_rows(dev):
    from fieldconv_amd.geodesic import geodesic_distances, mesh_edge_graph
    pos, face, sources, label, dist = surface_case()
    check_nearest(dev, pos, face, sources, label, dist)
    rows_src = gref.spread(400, 32, seed=5)
    want = gref.rows(pos, face, rows_src)
    p, f = T(pos, dev), T(face, dev)
    got, sweeps = geodesic_distances(p, f, T(rows_src, dev), return_sweeps=True)
    assert got.shape == (32, 400) and same_bits(got, want) and (N_(sweeps) >= 2).all()
    # chunked launches and a prebuilt graph give the same rows
    graph = mesh_edge_graph(p, f)
    assert torch.equal(geodesic_distances(p, f, T(rows_src, dev), graph=graph, rows_per_call=5), got)
    check_nearest(dev, pos, face, sources, label, dist, graph=graph)


def test_disconnected_and_faceless_vertices(dev):
    a, b = gref.lattice(5, 6), gref.lattice(4, 4)
    pos, face, _ = gref.union([a, b])
    pos = np.concatenate((pos, np.array([[9, 9, 9]], dtype=np.float32)))           # vertex 46: in no face
    sources = np.array([7, 0, 22], dtype=np.int64)                                  # all in the first component
    label, dist = gref.nearest(pos, face, sources)
    assert np.isinf(dist[30:]).all() and (label[30:] == -1).all() and np.isfinite(dist[:30]).all()
    check_nearest(dev, pos, face, sources, label, dist)
    from fieldconv_amd.geodesic import geodesic_distances
    row = geodesic_distances(T(pos, dev), T(face, dev), T(np.array([46, 31]), dev))
    assert same_bits(row, gref.rows(pos, face, [46, 31])) and float(row[0, 46]) == 0 and bool(torch.isinf(row[0, :46]).all())


def test_duplicate_sources_and_zero_length_edges(dev):
    pos, face = gref.lattice(6, 6)
    # vertex 36 sits on vertex 14 and is joined to it (and to 15) by a face: the edge 14 - 36 has length 0, tight both ways
    pos = np.concatenate((pos, pos[14:15]))
    face = np.concatenate((face, np.array([[14], [36], [15]])), 1)
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert (length == 0).sum() == 2
    for sources in ([20, 3, 20, 33], [36, 3, 14], [14, 3, 36], [5, 5]):
        sources = np.array(sources, dtype=np.int64)
        label, dist = gref.nearest(pos, face, sources)
        check_nearest(dev, pos, face, sources, label, dist)
    label, _ = gref.nearest(pos, face, np.array([20, 3, 20, 33]))
    assert label[20] == 0 and 2 not in label            # of a vertex listed twice the lower position counts
    label, dist = gref.nearest(pos, face, np.array([3, 30]))
    assert dist[36] == dist[14] and label[36] == label[14]


@pytest.mark.parametrize('extra', [0, 1])
def test_lds_boundary(dev, extra):
    """a strip with exactly the LDS capacity in vertices (solved in LDS) and one with a vertex more (the global-memory
    instantiation of the same loop)"""
    from fieldconv_amd.geodesic import LDS_VERTICES
    assert LDS_VERTICES == 20000
    nx, ny = ((10000, 2), (6667, 3))[extra]
    assert nx * ny == LDS_VERTICES + extra
    pos, face, sources, label, dist = lattice_case(nx, ny, 64)
    check_nearest(dev, pos, face, sources, label, dist)
    from fieldconv_amd.geodesic import geodesic_distances
    one = sources[:1]
    ptr, nbr, length = gref.edge_graph(pos, face)
    assert same_bits(geodesic_distances(T(pos, dev), T(face, dev), T(one, dev)), gref.dijkstra32(ptr, nbr, length, one)[None])


@pytest.mark.parametrize('shape', [(33, 31), (32, 32), (25, 41), (3, 1)])
def test_workgroup_remainder(dev, shape):
    if shape == (3, 1):
        pos = np.array([[0, 0, 0], [1, 0, 0], [0, 0.75, 0]], dtype=np.float32)
        face = np.array([[0], [1], [2]], dtype=np.int64)
        sources = np.array([2], dtype=np.int64)
        label, dist = gref.nearest(pos, face, sources)
    else:
        assert shape[0] * shape[1] in (1023, 1024, 1025)
        pos, face, sources, label, dist = lattice_case(shape[0], shape[1], 5)
    check_nearest(dev, pos, face, sources, label, dist)


def _batch(meshes, n_samples):
    pos, face, pos_ptr = gref.union(meshes)
    samples = [gref.spread(m[0].shape[0], n, seed=k) for k, (m, n) in enumerate(zip(meshes, n_samples))]
    sample_ptr = np.cumsum([0] + list(n_samples)).astype(np.int64)
    return pos, face, pos_ptr, samples, sample_ptr


@pytest.mark.parametrize('large_first', [False, True])
def test_batch_equals_single_calls(dev, large_first):
    """three meshes through the ptr tables = the three single calls with labels offset; once with a first mesh over the LDS
    capacity (one launch of each instantiation)"""
    from fieldconv_amd.geodesic import nearest_sample, sample_weights
    first = gref.lattice(6667, 3) if large_first else gref.lattice(7, 9)
    meshes = [first, gref.surface(400, seed=1), gref.lattice(5, 4)]
    n_samples = [11, 9, 3]
    pos, face, pos_ptr, samples, sample_ptr = _batch(meshes, n_samples)
    union_idx = np.concatenate([s + o for s, o in zip(samples, pos_ptr[:-1])])
    label, dist, sweeps = nearest_sample(T(pos, dev), T(face, dev), T(union_idx, dev), T(pos_ptr, dev), T(sample_ptr, dev), return_sweeps=True)
    assert sweeps.shape == (3, 2) and (N_(sweeps) >= 1).all()
    w = sample_weights(T(pos, dev), T(face, dev), T(union_idx, dev), T(pos_ptr, dev), T(sample_ptr, dev))
    for b, (m, s) in enumerate(zip(meshes, samples)):
        v0, v1 = pos_ptr[b], pos_ptr[b + 1]
        want_label, want_dist = gref.nearest(m[0], m[1], s)
        one_label, one_dist = nearest_sample(T(m[0], dev), T(m[1], dev), T(s, dev))
        assert np.array_equal(N_(one_label), want_label) and same_bits(one_dist, want_dist)
        assert np.array_equal(N_(label[v0:v1]), want_label + sample_ptr[b]) and same_bits(dist[v0:v1], want_dist)
        one_w = sample_weights(T(m[0], dev), T(m[1], dev), T(s, dev))
        assert torch.equal(w[sample_ptr[b]:sample_ptr[b + 1]], one_w)


def test_batch_rejects_samples_of_another_mesh(dev):
    from fieldconv_amd.geodesic import nearest_sample
    pos, face, pos_ptr, samples, sample_ptr = _batch([gref.lattice(4, 4), gref.lattice(3, 5)], [2, 2])
    wrong = np.concatenate((samples[0], samples[1]))            # the second mesh's samples not offset: rows of the first
    with pytest.raises(ValueError):
        nearest_sample(T(pos, dev), T(face, dev), T(wrong, dev), T(pos_ptr, dev), T(sample_ptr, dev))


# ------------------------------------------------------------------ weights, maps, the error metric
def test_sample_weights(dev):
    from fieldconv_amd.geodesic import sample_weights, vertex_masses
    pos, face, sources, label, _ = surface_case()
    p, f, s = T(pos, dev), T(face, dev), T(sources, dev)
    assert same_bits(vertex_masses(p, f), gref.vertex_masses(pos, face))
    w = sample_weights(p, f, s)
    assert w.shape == (9, 1) and same_bits(w, gref.sample_weights(pos, face, label, 9))
    area = gref.area64(pos, face)
    assert abs(float(w.double().sum()) - area) <= 1e-6 * area          # a connected mesh: every vertex's mass lands on a sample
    assert torch.equal(sample_weights(p, f, s), w)                      # fixed-order sums: the same bits again
    # unreachable vertices contribute to nothing
    a, b = gref.lattice(5, 6), gref.lattice(4, 4)
    upos, uface, _ = gref.union([a, b])
    src = np.array([7, 0], dtype=np.int64)
    ulabel, _ = gref.nearest(upos, uface, src)
    uw = sample_weights(T(upos, dev), T(uface, dev), T(src, dev))
    assert same_bits(uw, gref.sample_weights(upos, uface, ulabel, 2))
    assert abs(float(uw.double().sum()) - gref.area64(*a)) <= 1e-6 * gref.area64(*a)


def test_sample_weights_transform_feeds_fc_precomp(dev):
    """SupportGraph -> SampleWeights -> FCPrecomp on a synthetic mesh, single and as a MeshBatch"""
    from types import SimpleNamespace
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.transforms import FCPrecomp, SampleWeights, SupportGraph
    pos, face, *_ = surface_case()

    def run(data):
        data = SampleWeights()(SupportGraph(epsilon=0.3, sample_n=64, random_start=False)(data))
        S, E = data.sample_idx.shape[0], data.supp_edges.shape[0]
        assert data.w.shape == (S, 1) and data.w.dtype == torch.float32 and bool((data.w > 0).all())
        g = torch.Generator().manual_seed(0)
        data.logMag = (0.3 * torch.rand(E, generator=g)).to(dev)
        data.logAng = (6.28 * torch.rand(E, generator=g)).to(dev)
        ang = 6.28 * torch.rand(E, generator=g)
        data.xp = torch.polar(torch.ones(E), ang).to(dev)
        edges, sten, ln, wxp = FCPrecomp(band_limit=1, n_rings=3, epsilon=0.3)(data)
        assert 0 < edges.shape[0] <= E and tuple(sten.shape) == (edges.shape[0], 3, 3) and bool(torch.isfinite(wxp.abs()).all())
        return data.w

    single = run(SimpleNamespace(pos=T(pos, dev), face=T(face, dev)))
    meshes = [SimpleNamespace(pos=torch.from_numpy(pos), face=torch.from_numpy(face)) for _ in range(2)]
    batched = run(MeshBatch.from_list(meshes).to(dev))
    assert torch.equal(batched, torch.cat((single, single)))


def test_samples_to_nearest_and_compose_map(dev):
    from fieldconv_amd.geodesic import compose_map, samples_to_nearest
    pos, face, sources, label, _ = surface_case()
    assert np.array_equal(N_(samples_to_nearest(T(pos, dev), T(face, dev), T(sources, dev))), label)
    # template vertex l sits on source vertex tem2sour[l] - 1 and carries target label tem2tar[l]; vertex 17 is hit twice
    rng = np.random.default_rng(3)
    hit = rng.permutation(400)[:120]
    tem2sour = np.concatenate((hit, [hit[17]])) + 1
    tem2tar = rng.integers(1, 5000, size=121)
    got = N_(compose_map(T(tem2tar, dev), T(tem2sour, dev), T(pos, dev), T(face, dev)))
    want = np.zeros(400, dtype=np.int64)
    last = {}
    for l, v in enumerate(tem2sour - 1):
        last[v] = l
    srcs = np.array(sorted(last), dtype=np.int64)
    near, _ = gref.nearest(pos, face, srcs)
    for v in range(400):
        want[v] = tem2tar[last[srcs[near[v]]]]
    assert np.array_equal(got, want) and got[hit[17]] == tem2tar[120]


def test_geodesic_error_and_curve(dev):
    from fieldconv_amd.geodesic import correspondence_curve, geodesic_distances, geodesic_error
    pos, face, *_ = surface_case()
    p, f = T(pos, dev), T(face, dev)
    rng = np.random.default_rng(4)
    target = rng.integers(0, 400, size=300)
    pred = np.where(rng.random(300) < 0.5, target, rng.integers(0, 400, size=300))
    full = geodesic_distances(p, f, torch.arange(400, device=dev))
    want = full[T(target, dev), T(pred, dev)]
    raw = geodesic_error(p, f, T(pred, dev), T(target, dev), normalize=False)
    assert raw.dtype == torch.float32 and torch.equal(raw, want)
    assert torch.equal(geodesic_error(p, f, T(pred, dev), T(target, dev), normalize=False, rows_per_call=7), want)
    assert bool((raw[T(pred == target, dev)] == 0).all()) and bool((raw[T(pred != target, dev)] > 0).all())
    # normalised: one float32 division by sqrt(area); the area sums float32 triangle areas (4 ulp covers the two roundings)
    err = geodesic_error(p, f, T(pred, dev), T(target, dev))
    scale = np.float32(np.sqrt(gref.face_areas(pos, face).astype(np.float64).sum()))
    assert np.allclose(N_(err), N_(want) / scale, rtol=4 * 2.0 ** -24, atol=0)
    ts = [0.0, 0.02, 0.05, 0.1, 0.25, 10.0]
    curve = correspondence_curve(err, ts)
    assert np.array_equal(N_(curve), np.array([(N_(err) <= np.float32(t)).mean() for t in ts]))
    assert curve[0] >= 0.5 - 0.1 and curve[-1] == 1.0


def test_cpu_tensors_in_cpu_tensors_out(dev):
    from fieldconv_amd import geodesic as G
    pos, face, sources, label, dist = surface_case()
    p, f, s = torch.from_numpy(pos), torch.from_numpy(face), torch.from_numpy(sources)
    got_label, got_dist = G.nearest_sample(p, f, s)
    assert not got_label.is_cuda and not got_dist.is_cuda
    assert np.array_equal(got_label.numpy(), label) and same_bits(got_dist, dist)
    graph = G.mesh_edge_graph(p, f)
    assert all(not t.is_cuda for t in graph)
    rows = G.geodesic_distances(p, f, s, graph=graph, rows_per_call=4)
    assert not rows.is_cuda and same_bits(rows, gref.rows(pos, face, sources))
    w = G.sample_weights(p, f, s)
    assert not w.is_cuda and same_bits(w, gref.sample_weights(pos, face, label, 9))
    assert not G.geodesic_error(p, f, s, s).is_cuda and not G.compose_map(s + 1, s + 1, p, f).is_cuda
