"""Geodesic farthest-point sampling and geodesic-ball support edges on the device (fieldconv_amd.geodesic_sampling,
csrc/fc_geodesic_fps.hip) against the numpy restatement tests/_geodesic_sampling_ref.py: indices equal, distances bit for bit
-- everything is a function of least fixpoints, so there is nothing to tolerate.  Shapes sit where the kernels can go wrong:
exact ties (a binary lattice, a threshold that distances hit exactly), an irregular surface, further components, faceless
vertices and zero-length edges, sizes around the 1024 threads of the workgroup, the LDS capacity and one vertex more (the
global-memory instantiation), and batches that mix both instantiations."""
import functools

import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref

pytestmark = pytest.mark.gpu

CAP = 20000
STRIPS = {CAP: (10000, 2), CAP + 1: (6667, 3)}


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
    'cap': lambda: gref.lattice(*STRIPS[CAP]), 'cap+1': lambda: gref.lattice(*STRIPS[CAP + 1]),
    'l79': lambda: gref.lattice(7, 9), 'l54': lambda: gref.lattice(5, 4),
}


# every reference is computed once and shared (the tests only read it)
@functools.lru_cache(maxsize=None)
def mesh(name):
    return MESHES[name]()


@functools.lru_cache(maxsize=None)
def fps_case(name, n_samples, start):
    pos, face = mesh(name)
    return (pos, face) + sref.mesh_fps(pos, face, n_samples, start)


@functools.lru_cache(maxsize=None)
def ball_case(name, epsilon, k=512):
    """the 64 sorted samples of the mesh's sampling case and their ball edges"""
    pos, face, idx, _ = fps_case(name, 64, 5)
    samples = np.sort(idx)
    return (pos, face, samples) + sref.mesh_ball_edges(pos, face, samples, epsilon, k)


def check_fps(dev, name, n_samples, start):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample
    pos, face, want_idx, want_d = fps_case(name, n_samples, start)
    idx, dist, sweeps = geodesic_farthest_point_sample(T(pos, dev), T(face, dev), n_samples, start, return_dist=True, return_sweeps=True)
    assert idx.dtype == torch.int64 and idx.device == dev and dist.device == dev
    assert np.array_equal(N_(idx), want_idx)
    assert same_bits(dist, want_d)
    assert int(sweeps) >= n_samples          # every round ends in a sweep that changes nothing
    return idx, dist


# ------------------------------------------------------------------ sampling
def test_fps_lattice_with_exact_ties(dev):
    pos, face, idx, d = fps_case('lattice', 64, 5)
    ptr, nbr, length = gref.edge_graph(pos, face)
    tied = []

    def count_ties(k, taken, field):
        free = np.setdiff1d(np.arange(len(field)), taken)
        tied.append(int((field[free] == field[free].max()).sum()) > 1)
    sref.fps(ptr, nbr, length, 64, 5, each_round=count_ties)
    assert sum(tied) >= 8, 'the lattice must tie for the next choice in many rounds'
    check_fps(dev, 'lattice', 64, 5)


def test_fps_takes_every_vertex_exactly_once(dev):
    idx, dist = check_fps(dev, 'small_lattice', 30, 0)
    assert sorted(N_(idx).tolist()) == list(range(30)) and bool((dist == 0).all())


def test_fps_irregular_surface(dev):
    check_fps(dev, 'surface', 64, 0)


def test_fps_components_faceless_and_duplicated_vertices(dev):
    """+inf is picked first, lowest number first; the zero-length edge leaves d = 0 on a vertex not taken, which is still
    taken exactly once"""
    idx, _ = check_fps(dev, 'odd', 12, 7)
    assert N_(idx)[:3].tolist() == [7, 30, 46]
    idx, dist = check_fps(dev, 'odd', 48, 7)
    assert sorted(N_(idx).tolist()) == list(range(48))


@pytest.mark.parametrize('name', ['v1023', 'v1024', 'v1025'])
def test_fps_workgroup_remainder(dev, name):
    check_fps(dev, name, 8, 0)


@pytest.mark.parametrize('name', ['cap', 'cap+1'])
def test_fps_lds_boundary(dev, name):
    """a strip with exactly the LDS capacity in vertices and one with a vertex more: both instantiations of the kernel"""
    from fieldconv_amd.geodesic_sampling import LDS_VERTICES
    assert LDS_VERTICES == CAP and mesh(name)[0].shape[0] == CAP + (name == 'cap+1')
    check_fps(dev, name, 8, 0)


def test_fps_batch_equals_single_calls(dev):
    """four meshes, the second above the LDS capacity (one launch of each instantiation), with their own counts and starts"""
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample, geodesic_farthest_point_sample_batched
    names, counts, starts = ['l79', 'cap+1', 'surface300', 'l54'], [11, 8, 9, 3], [3, 0, 0, 2]
    pos, face, pos_ptr = gref.union([mesh(n) for n in names])
    idx, dist, sweeps = geodesic_farthest_point_sample_batched(T(pos, dev), T(face, dev), T(pos_ptr, dev), counts, starts, return_dist=True,
                                                               return_sweeps=True)
    assert idx.shape == (sum(counts),) and sweeps.shape == (4,)
    out = np.cumsum([0] + counts)
    for b, name in enumerate(names):
        p, f, want_idx, want_d = fps_case(name, counts[b], starts[b])
        one, one_sweeps = geodesic_farthest_point_sample(T(p, dev), T(f, dev), counts[b], starts[b], return_sweeps=True)
        assert np.array_equal(N_(one), want_idx)
        assert np.array_equal(N_(idx[out[b]:out[b + 1]]), want_idx)          # local to the mesh, in selection order
        assert same_bits(dist[pos_ptr[b]:pos_ptr[b + 1]], want_d)
        assert int(sweeps[b]) >= counts[b]
    same = geodesic_farthest_point_sample_batched(T(pos, dev), T(face, dev), T(pos_ptr, dev), 3)          # one count for all
    assert np.array_equal(N_(same).reshape(4, 3), np.stack([fps_case(n, 3, 0)[2] for n in names]))


def test_fps_field_is_todays_nearest_sample_field(dev):
    """the new kernel's final field against the existing one's, on the device"""
    from fieldconv_amd.geodesic import mesh_edge_graph, nearest_sample
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample
    for name in ('surface', 'odd'):
        pos, face = mesh(name)
        p, f = T(pos, dev), T(face, dev)
        graph = mesh_edge_graph(p, f)
        idx, dist = geodesic_farthest_point_sample(p, f, 40, 3, graph=graph, return_dist=True)
        assert torch.equal(dist.view(torch.int32), nearest_sample(p, f, idx)[1].view(torch.int32))
        assert torch.equal(idx, geodesic_farthest_point_sample(p, f, 40, 3))          # with and without the prebuilt graph
        for k in (1, 7, 39):          # a prefix of the selection is the selection of fewer rounds, and its field is d_k
            head, d_k = geodesic_farthest_point_sample(p, f, k, 3, graph=graph, return_dist=True)
            assert torch.equal(head, idx[:k]) and torch.equal(d_k.view(torch.int32), nearest_sample(p, f, idx[:k])[1].view(torch.int32))


def test_two_runs_give_the_same_result(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample, geodesic_radius_edges
    pos, face = mesh('surface')
    p, f = T(pos, dev), T(face, dev)
    # (the sweep COUNT may differ between runs: a pull may or may not see what a neighbour wrote in the same sweep; the fixpoint cannot)
    a = geodesic_farthest_point_sample(p, f, 64, 0, return_dist=True)
    b = geodesic_farthest_point_sample(p, f, 64, 0, return_dist=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))
    s = a[0].sort()[0]
    ea, eb = geodesic_radius_edges(p, f, s, 0.2, return_dist=True), geodesic_radius_edges(p, f, s, 0.2, return_dist=True)
    assert torch.equal(ea[0], eb[0]) and torch.equal(ea[1].view(torch.int32), eb[1].view(torch.int32))


def test_cpu_tensors_in_cpu_tensors_out(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample, geodesic_radius_edges
    pos, face, want_idx, want_d = fps_case('lattice', 64, 5)
    idx, dist = geodesic_farthest_point_sample(torch.from_numpy(pos), torch.from_numpy(face), 64, 5, return_dist=True)
    assert not idx.is_cuda and not dist.is_cuda and np.array_equal(idx.numpy(), want_idx) and same_bits(dist, want_d)
    _, _, samples, want_e, _ = ball_case('lattice', 0.375)
    edges = geodesic_radius_edges(torch.from_numpy(pos), torch.from_numpy(face), torch.from_numpy(samples), 0.375)
    assert not edges.is_cuda and np.array_equal(edges.numpy(), want_e)


# ------------------------------------------------------------------ balls
def check_ball(dev, name, epsilon, k=512):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face, samples, want_e, want_d = ball_case(name, epsilon, k)
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(samples, dev), epsilon, k, return_dist=True)
    assert edges.dtype == torch.int64 and edges.device == dev and tuple(edges.shape) == want_e.shape
    assert np.array_equal(N_(edges), want_e)
    assert same_bits(dist, want_d)
    assert torch.equal(geodesic_radius_edges(T(pos, dev), T(face, dev), T(samples, dev), epsilon, k), edges)
    return edges, dist


def test_ball_lattice_excludes_distances_equal_to_epsilon(dev):
    """epsilon = 3 h is exactly representable and sample pairs lie at exactly that distance: the comparison is strict"""
    pos, face, samples, want_e, want_d = ball_case('lattice', 0.375)
    rows = gref.rows(pos, face, samples)[:, samples]
    assert (rows == np.float32(0.375)).any() and len(want_e) == (rows < np.float32(0.375)).sum()
    edges, dist = check_ball(dev, 'lattice', 0.375)
    # the distances are the bits of geodesic_distances' rows
    from fieldconv_amd.geodesic import geodesic_distances
    full = geodesic_distances(T(pos, dev), T(face, dev), T(samples, dev))[:, T(samples, dev)]
    assert torch.equal(dist.view(torch.int32), full[edges[:, 0], edges[:, 1]].view(torch.int32))


def test_ball_irregular_surface(dev):
    pos, face, samples, want_e, _ = ball_case('surface', 0.2)
    assert len(want_e) > 3 * 64
    check_ball(dev, 'surface', 0.2)


def test_ball_cap_keeps_the_nearest_by_distance_then_position(dev):
    pos, face, samples, want_e, want_d = ball_case('lattice', 0.375, 4)
    full_e, full_d = ball_case('lattice', 0.375)[3:]
    counts = np.bincount(full_e[:, 0], minlength=64)
    assert (counts > 4).any() and (np.bincount(want_e[:, 0], minlength=64) == np.minimum(counts, 4)).all()
    # a query whose cut falls between equal distances: the position decides
    cut_in_tie = False
    for q in np.nonzero(counts > 4)[0]:
        d_all, d_kept = np.sort(full_d[full_e[:, 0] == q]), np.sort(want_d[want_e[:, 0] == q])
        cut_in_tie |= d_all[4] == d_kept[3]
    assert cut_in_tie, 'the lattice must cut inside a tie'
    check_ball(dev, 'lattice', 0.375, 4)


def test_ball_batch_equals_single_calls(dev):
    """three meshes through the ptr tables, the second above the LDS capacity: the rows of each mesh alone plus its offset"""
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    names = ['l79', 'cap+1', 'surface300']
    local = [np.sort(fps_case('l79', 11, 3)[2]), CLUSTERED, np.sort(fps_case('surface300', 9, 0)[2])]
    eps = 0.3
    pos, face, pos_ptr = gref.union([mesh(n) for n in names])
    sample_ptr = np.cumsum([0] + [len(s) for s in local]).astype(np.int64)
    union_idx = np.concatenate([s + o for s, o in zip(local, pos_ptr[:-1])])
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(union_idx, dev), eps, pos_ptr=T(pos_ptr, dev),
                                        sample_ptr=T(sample_ptr, dev), return_dist=True)
    want_e, want_d = [], []
    for b, name in enumerate(names):
        p, f = mesh(name)
        e, d = sref.mesh_ball_edges(p, f, local[b], eps)
        one_e, one_d = geodesic_radius_edges(T(p, dev), T(f, dev), T(local[b], dev), eps, return_dist=True)
        assert np.array_equal(N_(one_e), e) and same_bits(one_d, d)
        want_e.append(e + sample_ptr[b])
        want_d.append(d)
    assert np.array_equal(N_(edges), np.concatenate(want_e)) and same_bits(dist, np.concatenate(want_d))


# eight samples of the strip above the LDS capacity, some within reach of each other and some at exactly 3 h
CLUSTERED = np.array([0, 4, 9, 3000, 3003, 10000, 10001, 20000], dtype=np.int64)


def test_ball_above_the_lds_capacity(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face = mesh('cap+1')
    want_e, want_d = sref.mesh_ball_edges(pos, face, CLUSTERED, 0.375)
    assert 8 < len(want_e) < 64
    edges, dist = geodesic_radius_edges(T(pos, dev), T(face, dev), T(CLUSTERED, dev), 0.375, return_dist=True)
    assert np.array_equal(N_(edges), want_e) and same_bits(dist, want_d)


def test_ball_rejects_samples_that_do_not_ascend(dev):
    from fieldconv_amd.geodesic_sampling import geodesic_radius_edges
    pos, face = mesh('l79')
    for bad in ([5, 3, 9], [3, 5, 5]):
        with pytest.raises(ValueError):
            geodesic_radius_edges(T(pos, dev), T(face, dev), T(np.array(bad, dtype=np.int64), dev), 0.3)


# ------------------------------------------------------------------ the transform
def test_transform_equals_composing_the_pieces(dev):
    from types import SimpleNamespace
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.geodesic_sampling import geodesic_farthest_point_sample, geodesic_radius_edges
    from fieldconv_amd.transforms import GeodesicSupportGraph, SampleWeights
    pos, face = mesh('surface300')
    p, f = T(pos, dev), T(face, dev)
    data = GeodesicSupportGraph(epsilon=0.3, sample_n=64, random_start=False)(SimpleNamespace(pos=p, face=f))
    want_idx = geodesic_farthest_point_sample(p, f, 64, 0).sort()[0]
    want_edges = geodesic_radius_edges(p, f, want_idx, 0.3)
    assert torch.equal(data.sample_idx, want_idx) and torch.equal(data.supp_edges, want_edges)
    assert np.array_equal(N_(want_idx), np.sort(fps_case('surface300', 64, 0)[2]))
    data = SampleWeights()(data)
    assert data.w.shape == (64, 1) and bool((data.w > 0).all())
    # a random start is drawn from the generator, as in SupportGraph
    g = torch.Generator().manual_seed(7)
    start = int(torch.randint(300, (1,), generator=torch.Generator().manual_seed(7)))
    drawn = GeodesicSupportGraph(epsilon=0.3, sample_n=16, generator=g)(SimpleNamespace(pos=p, face=f))
    assert torch.equal(drawn.sample_idx, geodesic_farthest_point_sample(p, f, 16, start).sort()[0])
    # sample_n above V, or none: every vertex; a sample_idx that is already there is kept
    every = GeodesicSupportGraph(epsilon=0.1, sample_n=1000)(SimpleNamespace(pos=p, face=f))
    assert torch.equal(every.sample_idx, torch.arange(300, device=dev))
    kept = GeodesicSupportGraph(epsilon=0.3)(SimpleNamespace(pos=p, face=f, sample_idx=want_idx[::2].contiguous()))
    assert torch.equal(kept.supp_edges, geodesic_radius_edges(p, f, want_idx[::2].contiguous(), 0.3))

    # a MeshBatch: mesh for mesh the single call, offset
    other = mesh('l79')
    meshes = [SimpleNamespace(pos=torch.from_numpy(pos), face=torch.from_numpy(face)),
              SimpleNamespace(pos=torch.from_numpy(other[0]), face=torch.from_numpy(other[1]))]
    batch = SampleWeights()(GeodesicSupportGraph(epsilon=0.3, sample_n=64, random_start=False)(MeshBatch.from_list(meshes).to(dev)))
    second = GeodesicSupportGraph(epsilon=0.3, sample_n=64, random_start=False)(SimpleNamespace(pos=T(other[0], dev), face=T(other[1], dev)))
    assert second.sample_idx.shape[0] == 63          # min(sample_n, n_b)
    assert torch.equal(batch.sample_idx, torch.cat((want_idx, second.sample_idx + 300)))
    assert batch.ptr.tolist() == [0, 64, 127] and batch.edge_ptr.tolist() == [0, want_edges.shape[0], want_edges.shape[0] + second.supp_edges.shape[0]]
    assert torch.equal(batch.supp_edges, torch.cat((want_edges, second.supp_edges + 64)))
    assert torch.equal(batch.batch, torch.cat((torch.zeros(64), torch.ones(63))).to(batch.batch))
    assert torch.equal(batch.w[:64], data.w)
