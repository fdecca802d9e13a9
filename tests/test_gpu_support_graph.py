"""Support-graph kernels (csrc/fc_support.hip) against a numpy float32 restatement of their contract: farthest-point
sampling index for index, radius neighbours as the whole (E,2) tensor in order, the SupportGraph transform end to end, and
a support graph built here feeding FCPrecomp and a FieldConv forward.

The restatement evaluates d2 = (dx*dx + dy*dy) + dz*dz in float32, each operation rounded on its own, which is what the
kernels compute; for large point sets the candidates come from a cKDTree with a slightly larger radius and are re-filtered
with the exact float32 rule."""
import math

import numpy as np
import pytest
import torch
from scipy.spatial import cKDTree

from conftest import rel_err
from oracle import fieldconv_oracle as orc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


# ---------------------------------------------------------------- the restatement
def sq_dist(p, q):
    """float32 squared distances of the rows of p (M,3) to the point q (3,) (or to the rows of q (M,3))."""
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps_ref(p, S, start):
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = p.shape[0]
    mind = np.full(N, np.inf, dtype=np.float32)
    taken = np.zeros(N, dtype=bool)
    out = np.empty(S, dtype=np.int64)
    last = start
    for k in range(S):
        out[k] = last
        taken[last] = True
        if k + 1 == S:
            break
        np.minimum(mind, sq_dist(p, p[last]), out=mind)
        last = int(np.argmax(np.where(taken, np.float32(-1), mind)))        # first maximum: the lowest index
    return out


def _truncate(q, n, d2, K):
    """Keep, per query, the K smallest (d2, n); return the rows sorted by (q, n)."""
    order = np.lexsort((n, d2, q))
    q, n = q[order], n[order]
    first = np.searchsorted(q, q, side='left')
    keep = (np.arange(q.size) - first) < K
    q, n = q[keep], n[keep]
    order = np.lexsort((n, q))
    return np.stack((q[order], n[order]), 1).astype(np.int64)


def radius_ref(p, eps, K):
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = p.shape[0]
    r2 = np.float32(eps) * np.float32(eps)
    if N <= 3000:
        d2 = sq_dist(p[None, :, :], p[:, None, :])                         # [q, n]: p_n - p_q
        q, n = np.nonzero(d2 < r2)
        return _truncate(q, n, d2[q, n], K)
    tree = cKDTree(p.astype(np.float64))
    pairs = tree.query_pairs(float(np.sqrt(np.float64(r2))) * (1 + 1e-4) + 1e-7, output_type='ndarray')
    q = np.concatenate((pairs[:, 0], pairs[:, 1], np.arange(N)))
    n = np.concatenate((pairs[:, 1], pairs[:, 0], np.arange(N)))
    d2 = sq_dist(p[n], p[q])
    m = d2 < r2
    return _truncate(q[m], n[m], d2[m], K)


# ---------------------------------------------------------------- point sets
def random_points(N, seed):
    return np.random.default_rng(seed).random((N, 3)).astype(np.float32)


def sphere_points(N, seed=0, jitter=0.15):
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / N
    rad = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    lon = math.pi * (3.0 - math.sqrt(5.0)) * i
    p = np.stack((rad * np.cos(lon), rad * np.sin(lon), z), 1)
    p = p + (jitter / math.sqrt(N)) * np.random.default_rng(seed).standard_normal((N, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def lattice(n):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing='ij'), -1).reshape(-1, 3).copy()


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ---------------------------------------------------------------- farthest-point sampling
FPS_N = [1, 2, 63, 64, 65, 1000, 6890, 20000, 160000]


def _fps_cases():
    cases = []
    for N in FPS_N:
        for S in sorted({1, max(1, N // 7), min(1024, N), N}):
            if N == 160000 and S > 1024:
                continue        # O(N S) restatement: minutes of numpy at S = 22 857 / 160 000 (the kernel itself is exercised at 20 000)
            cases.append((N, S))
    return cases


@pytest.mark.parametrize('N,S', _fps_cases(), ids=lambda v: str(v))
def test_fps_equals_restatement(N, S, dev):
    p = sphere_points(N, seed=N) if N % 2 == 0 else random_points(N, seed=N)
    from fieldconv_amd.transforms import farthest_point_sample
    starts = sorted({0, N - 1, (N * 37) // 100})
    for start in starts:
        got = farthest_point_sample(T(p, dev), S, start)
        assert got.device == dev and got.dtype == torch.int64 and got.shape == (S,)
        ref = fps_ref(p, S, start)
        assert np.array_equal(got.cpu().numpy(), ref), (N, S, start)


def test_fps_duplicates_never_repeat(dev):
    from fieldconv_amd.transforms import farthest_point_sample
    base = random_points(300, seed=5)
    p = np.concatenate((base, base, base[:100], np.zeros((50, 3), np.float32)))        # every position at least twice
    N = p.shape[0]
    for S in (10, 400, N):
        got = farthest_point_sample(T(p, dev), S, 3).cpu().numpy()
        assert np.unique(got).size == S
        assert np.array_equal(got, fps_ref(p, S, 3))
    assert np.array_equal(np.sort(got), np.arange(N))                                  # S = N: a permutation
    # all points at one position: still a permutation, in index order after the start
    same = np.ones((70, 3), np.float32)
    got = farthest_point_sample(T(same, dev), 70, 5).cpu().numpy()
    assert np.array_equal(got, np.concatenate(([5], np.delete(np.arange(70), 5))))


def test_fps_is_bitwise_repeatable_and_keeps_the_input_device(dev):
    from fieldconv_amd.transforms import farthest_point_sample
    p = sphere_points(20000, seed=9)
    a = farthest_point_sample(T(p, dev), 2000, 17)
    b = farthest_point_sample(T(p, dev), 2000, 17)
    assert torch.equal(a, b)
    c = farthest_point_sample(torch.from_numpy(p), 2000, 17)                # CPU in, CPU out, same indices
    assert c.device.type == 'cpu' and torch.equal(c, a.cpu())


# ---------------------------------------------------------------- radius neighbours
def _check_radius(p, eps, K, dev):
    from fieldconv_amd.transforms import radius_edges
    got = radius_edges(T(p, dev), eps, K)
    assert got.device == dev and got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2
    ref = radius_ref(p, eps, K)
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got, ref)
    return got


@pytest.mark.parametrize('kind,N,eps,K', [
    ('random', 1, 0.1, 512), ('random', 300, 0.2, 512), ('random', 2000, 0.15, 512), ('random', 2000, 0.3, 20),
    ('sphere', 2500, 0.12, 512), ('sphere', 2500, 0.2, 9), ('sphere', 6890, 0.1, 512),
])
def test_radius_equals_restatement(kind, N, eps, K, dev):
    p = random_points(N, seed=N) if kind == 'random' else sphere_points(N, seed=N)
    got = _check_radius(p, eps, K, dev)
    assert np.all(got[got[:, 0] == got[:, 1], 0] == np.arange(N))            # every point is its own neighbour


@pytest.mark.parametrize('eps', [1.0, math.sqrt(2.0), math.sqrt(3.0), 2.0])
def test_radius_on_a_lattice_excludes_the_boundary(eps, dev):
    """Integer lattice: many squared distances equal r2 exactly (eps = 1, 2) and must be excluded."""
    p = lattice(9)
    got = _check_radius(p, eps, 512, dev)
    if eps == 1.0:
        assert np.array_equal(got, np.stack((np.arange(p.shape[0]),) * 2, 1))     # only the point itself


@pytest.mark.parametrize('K', [1, 7, 512])
def test_radius_overfull_keeps_the_nearest_with_index_ties(K, dev):
    p = lattice(10) if K < 512 else lattice(12)          # 1000 / 1728 points, every query sees all of them
    got = _check_radius(p, 100.0, K, dev)
    assert np.all(np.bincount(got[:, 0], minlength=p.shape[0]) == K)
    if K == 1:
        assert np.array_equal(got[:, 1], np.arange(p.shape[0]))
    # and a radius at which only part of the queries overflow
    _check_radius(p, 2.5, K, dev)


def test_radius_20000_in_full(dev):
    p = random_points(20000, seed=11)
    _check_radius(p, 0.07, 512, dev)
    _check_radius(p, 0.07, 16, dev)                      # ~30 candidates per query: most queries overfull


def test_radius_160000(dev):
    """Per-query counts of every query, and the lists of 2 000 sampled queries."""
    from fieldconv_amd.transforms import radius_edges
    p = random_points(160000, seed=12)
    got = radius_edges(T(p, dev), 0.035, 512).cpu().numpy()
    ref = radius_ref(p, 0.035, 512)
    assert np.array_equal(np.bincount(got[:, 0], minlength=160000), np.bincount(ref[:, 0], minlength=160000))
    assert np.all(np.diff(got[:, 0]) >= 0)
    off = np.concatenate(([0], np.cumsum(np.bincount(ref[:, 0], minlength=160000))))
    for q in np.random.default_rng(1).choice(160000, 2000, replace=False):
        assert np.array_equal(got[off[q]:off[q + 1]], ref[off[q]:off[q + 1]]), q


# ---------------------------------------------------------------- SupportGraph end to end
def icosphere_mesh(subdiv):
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
    v = np.array(verts) * np.array([1.3, 0.8, 1.0])          # an ellipsoid, so that NormalizeAxes has an order to find
    return torch.from_numpy(v.astype(np.float32)), torch.from_numpy(np.array(f, dtype=np.int64).T.copy())


def _normalised_mesh():
    from fieldconv_amd.transforms import NormalizeArea
    pos, face = icosphere_mesh(5)                            # 10 242 vertices
    return NormalizeArea()(Data(pos=pos, face=face))


def test_support_graph_transform_end_to_end(dev):
    from fieldconv_amd.transforms import SupportGraph
    mesh = _normalised_mesh()
    p = mesh.pos.numpy()
    N, eps = p.shape[0], 0.2
    # sample_n = 1024 from a fixed start, device data
    d = SupportGraph(eps, sample_n=1024, random_start=False)(Data(pos=mesh.pos.to(dev), face=mesh.face.to(dev)))
    samp = np.sort(fps_ref(p, 1024, 0))
    assert d.sample_idx.device == dev and np.array_equal(d.sample_idx.cpu().numpy(), samp)
    assert d.supp_edges.device == dev and np.array_equal(d.supp_edges.cpu().numpy(), radius_ref(p[samp], eps, 512))
    # CPU data: CPU outputs, equal to the device run
    c = SupportGraph(eps, sample_n=1024, random_start=False)(Data(pos=mesh.pos.clone(), face=mesh.face))
    assert c.sample_idx.device.type == 'cpu' and c.supp_edges.device.type == 'cpu'
    assert torch.equal(c.sample_idx, d.sample_idx.cpu()) and torch.equal(c.supp_edges, d.supp_edges.cpu())
    # a random start drawn from the generator
    start = int(torch.randint(N, (1,), generator=torch.Generator().manual_seed(4)))
    r = SupportGraph(eps, sample_n=500, generator=torch.Generator().manual_seed(4))(Data(pos=mesh.pos.clone()))
    assert np.array_equal(r.sample_idx.numpy(), np.sort(fps_ref(p, 500, start)))
    # a preset sample_idx is used as given
    preset = torch.arange(0, N, 7)
    e = SupportGraph(eps, sample_n=1024)(Data(pos=mesh.pos.clone(), sample_idx=preset))
    assert e.sample_idx is preset
    assert np.array_equal(e.supp_edges.numpy(), radius_ref(p[preset.numpy()], eps, 512))
    # sample_n > N keeps every point
    small = Data(pos=mesh.pos[:300].clone())
    s = SupportGraph(0.3, sample_n=301, max_num_neighbors=12)(small)
    assert torch.equal(s.sample_idx, torch.arange(300))
    assert np.array_equal(s.supp_edges.numpy(), radius_ref(p[:300], 0.3, 12))


def test_preprocessing_chain_feeds_fcprecomp_and_fieldconv(dev):
    """Edges of a unit-sphere sample from this package, closed-form log map and transport (fieldconv_amd.data.synthetic's
    formulas), then FCPrecomp and one FieldConv forward on the device against the oracle."""
    from fieldconv_amd.data.synthetic import _edge_fields, _frames
    from fieldconv_amd.nn import FieldConv
    from fieldconv_amd.transforms import FCPrecomp, SupportGraph
    from oracle.torch_composites import FCPrecomp as FCPrecompRef
    N, B, R, I, O = 3000, 2, 6, 16, 16
    pos = torch.from_numpy(sphere_points(N, seed=21))
    eps = 0.12
    d = SupportGraph(eps, sample_n=1500, random_start=False)(Data(pos=pos))
    pts = pos[d.sample_idx].numpy().astype(np.float64)
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    edges = d.supp_edges
    s, t = edges[:, 0].numpy(), edges[:, 1].numpy()
    e1, e2 = _frames(pts)
    dist, ang, xp_ang = _edge_fields(pts[s], e1[s], e2[s], pts[t], e1[t], e2[t])
    M = pts.shape[0]
    data = Data(supp_edges=edges, logMag=torch.from_numpy(dist).float(), logAng=torch.from_numpy(ang).float(),
                xp=torch.polar(torch.ones(dist.size), torch.from_numpy(xp_ang).float()),
                w=torch.full((M, 1), 4 * math.pi / M))
    eps_g = float(dist.max()) * 1.0001             # geodesic radius covering every edge
    ref_edges, ref_sten, _, _ = FCPrecompRef(B, R, eps_g)(data)
    dd = Data(**{k: v.to(dev) for k, v in data.__dict__.items()})
    e_dev, sten_dev, _, _ = FCPrecomp(B, R, eps_g)(dd)
    assert torch.equal(e_dev.cpu(), ref_edges)
    g = torch.Generator().manual_seed(5)
    x = torch.complex(torch.randn(M, I, generator=g), torch.randn(M, I, generator=g))
    conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=1).to(dev)
    y = conv(x.to(dev), e_dev, sten_dev)
    W = orc.effective_filter(conv.zonal.detach().cpu().numpy(), conv.spherical.detach().cpu().numpy(),
                             conv.phase.detach().cpu().numpy(), 1, B)
    y_ref = orc.fieldconv_forward(x.numpy(), ref_edges.numpy(), ref_sten.numpy(), W)
    assert rel_err(y.detach().cpu().numpy(), y_ref) < 1e-5
