"""Interpolation from the k nearest coarse samples on the device (csrc/fc_interp.hip, fieldconv_amd.transfer.interpolation_plan /
vertex_interpolation, nn.TangentInterpolate, transforms.CoarsenSamples(interpolate_k=...) / SamplesToVertices) against the numpy
restatement tests/_interp_ref.py.

The selection and the weights are float32 operations rounded one by one: bit for bit.  The candidate set is an integer decision
on fields that have the same bits everywhere: exact.  The operator is gated as tests/test_gpu_transfer.py gates it: against the
float64 restatement within 4 x the float32 restatement's own error, floor 1e-6 of the largest entry."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _geodesic_sampling_ref as sref
import _interp_ref as iref
import _logmap_ref as lref
import _transfer_ref as tref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev=torch.device('cuda:0')):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype in (np.float32, np.complex64) else a


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(bits(a), bits(b))


def gate_of(want64, own32):
    return max(4 * float(np.abs(own32 - want64).max()), 1e-6 * float(np.abs(want64).max()))


# ------------------------------------------------------------------ 1. the kernel on crafted rows
@pytest.mark.parametrize('power', [1, 2])
@pytest.mark.parametrize('k', [1, 3, 16])
def test_knn_weights_equal_the_restatement_bit_for_bit(dev, k, power):
    from fieldconv_amd.transfer import knn_weights
    rowptr, cand, dist = iref.crafted_csr(k)
    assert len(rowptr) == 301 and np.diff(rowptr)[5] == 200
    want_sel, want_w = iref.knn_weights(rowptr, cand, dist, k, power)
    args = (T(rowptr, dev), T(cand, dev), T(dist, dev), k, power)
    (sel, w), (sel2, w2) = knn_weights(*args), knn_weights(*args)
    assert sel.dtype == torch.int32 and w.dtype == torch.float32 and tuple(sel.shape) == tuple(w.shape) == (300, k)
    assert np.array_equal(N_(sel), want_sel)
    assert same_bits(N_(w), want_w)
    assert torch.equal(sel, sel2) and same_bits(N_(w), N_(w2))


def test_knn_weights_clamp_a_damaged_rowptr(dev):
    """entries outside [0, n_slots] and a descending pair read nothing outside the buffers: they are clamped as fc_transfer's"""
    from fieldconv_amd.transfer import knn_weights
    cand, dist = np.arange(6, dtype=np.int32), np.array([.5, .1, .3, .2, .6, .4], dtype=np.float32)
    rowptr = np.array([-5, 2, 1, 4, 2 ** 30], dtype=np.int32)                     # the rows read: [0,2), [2,2), [1,4), [4,6)
    sel, w = knn_weights(T(rowptr, dev), T(cand, dev), T(dist, dev), 3, 1)
    for f, (e0, e1) in enumerate(((0, 2), (2, 2), (1, 4), (4, 6))):
        want_sel, want_w = iref.knn_weights(np.array([e0, e1], dtype=np.int32), cand, dist, 3, 1)
        assert N_(sel)[f].tolist() == want_sel[0].tolist() and same_bits(N_(w)[f], want_w[0])
    assert N_(sel)[1].tolist() == [-1, -1, -1] and N_(sel)[3].tolist() == [5, 4, -1]


# ------------------------------------------------------------------ 2. plans on the icospheres
@functools.lru_cache(maxsize=None)
def ico_level(subdivisions, fine_kind):
    """(pos, face, fine sample_idx ascending, coarse positions ascending): 32 / 128 geodesic-FPS coarse samples of the 162- /
    642-vertex icosphere; fine: every vertex, or the first 4 x as many of the same FPS order (which begins with the coarse ones)"""
    pos, face = lref.icosphere(subdivisions)
    n = {2: 32, 3: 128}[subdivisions]
    order = sref.mesh_fps(pos, face, 4 * n, 0)[0]
    fine = np.arange(pos.shape[0]) if fine_kind == 'vertices' else np.sort(order)
    coarse = np.searchsorted(fine, np.sort(order[:n]))
    return pos, face, fine.astype(np.int64), coarse.astype(np.int64)


@functools.lru_cache(maxsize=None)
def ico_plan(subdivisions, fine_kind, diagonals):
    from fieldconv_amd.transfer import interpolation_plan
    pos, face, fine, coarse = ico_level(subdivisions, fine_kind)
    return interpolation_plan(T(pos), T(face), T(fine), T(coarse), diagonals=diagonals, return_rows=True)


@pytest.mark.parametrize('diagonals', [False, True])
@pytest.mark.parametrize('fine_kind', ['vertices', 'samples'])
@pytest.mark.parametrize('subdivisions', [2, 3])
def test_icosphere_plan_equals_the_restatement(dev, subdivisions, fine_kind, diagonals):
    pos, face, fine, coarse = ico_level(subdivisions, fine_kind)
    plan, rowptr, cand, dist, xp = ico_plan(subdivisions, fine_kind, diagonals)
    S_f, S_c = len(fine), len(coarse)
    assert (plan.n_out, plan.n_in) == (S_f, S_c) and not plan.conj_phase
    radius = iref.default_radius(pos, face, fine, coarse, diagonals)
    want_ptr, want_cand, field = iref.candidates(pos, face, fine, coarse, radius, diagonals)
    assert np.array_equal(N_(rowptr), want_ptr) and np.array_equal(N_(cand), want_cand)          # the candidate set, exactly
    assert np.diff(want_ptr).min() >= 1                                           # every fine sample has its own coarse sample at least
    # logMag is the unfolded length, the field the path's: the same geodesic seen twice, within a mesh cell of each other
    assert N_(dist).dtype == np.float32 and np.all(N_(dist) >= 0) and np.abs(N_(dist) - field).max() < 0.5 * radius
    sel, w = iref.knn_weights(N_(rowptr), N_(cand), N_(dist), 3, 2)
    rows, weight, phase = iref.plan_rows(N_(rowptr), N_(cand), N_(xp), sel, w)
    got_rows, got_w, got_ph = (N_(t) for t in plan.rows())
    assert np.array_equal(got_rows, rows) and same_bits(got_w, weight) and same_bits(got_ph, phase)
    assert plan.n_rows == len(rows) == int(np.minimum(np.diff(want_ptr), 3).sum())
    first = np.searchsorted(got_rows[:, 0], coarse)                                # a coarse sample's own rows: itself, 1, phase 1
    assert np.array_equal(got_rows[first, 1], np.arange(S_c)) and np.all(got_w[first] == 1) and np.all(got_ph[first] == 1)
    rest = np.setdiff1d(np.nonzero(np.isin(got_rows[:, 0], coarse))[0], first)    # and whatever follows it in that row weighs nothing
    assert np.all(got_w[rest] == 0)


def test_flat_grid_interpolation_is_a_convex_combination(dev):
    from fieldconv_amd.transfer import interpolation_plan, tangent_transfer
    pos, face = tref.flat_grid(12)
    coarse = np.array([13, 16, 19, 22, 49, 52, 55, 58, 85, 88, 91, 94, 121, 124, 127, 130], dtype=np.int64)
    plan = interpolation_plan(T(pos, dev), T(face, dev), torch.arange(144, device=dev), T(coarse, dev))
    rows, weight, phase = (N_(t) for t in plan.rows())
    assert np.abs(phase - 1).max() <= 1e-6                                         # all frames are equal
    h = (2 * pos[coarse, 0] + 3 * pos[coarse, 1] + 1).astype(np.float32)
    y = N_(tangent_transfer(T(h[:, None], dev), plan))[:, 0]
    lo, hi = np.full(144, np.inf), np.full(144, -np.inf)
    np.minimum.at(lo, rows[:, 0], h[rows[:, 1]])
    np.maximum.at(hi, rows[:, 0], h[rows[:, 1]])
    # three products and three additions rounded to float32, weights that sum to 1 within 3 x 2^-24: 9 roundings of the largest entry
    tol = 9 * 2.0 ** -24 * float(np.abs(h).max())
    assert np.all(np.isfinite(lo)) and np.all(y >= lo - tol) and np.all(y <= hi + tol)
    assert np.array_equal(y[coarse], h)                                            # exact at the coarse samples


# ------------------------------------------------------------------ 3. the operator
@functools.lru_cache(maxsize=None)
def operator_reference(complex_x, C, real):
    plan = ico_plan(2, 'vertices', False)[0]
    rows, weight, phase = (N_(t) for t in plan.rows())
    dt = np.complex64 if complex_x else np.float32
    x, gy = tref.features(plan.n_in, C, complex_x, 30 + C).astype(dt), tref.features(plan.n_out, C, complex_x, 40 + C).astype(dt)
    return (x, gy, tref.transfer(rows, weight, phase, False, plan.n_out, x, real),
            tref.adjoint(rows, weight, phase, False, plan.n_in, gy, real))


@pytest.mark.parametrize('C', [1, 5, 48])
@pytest.mark.parametrize('dtype', ['complex64', 'float32'])
def test_tangent_interpolate_forward_and_gradient(dev, dtype, C):
    from fieldconv_amd.nn import TangentInterpolate
    complex_x = dtype == 'complex64'
    level = SimpleNamespace(interp=ico_plan(2, 'vertices', False)[0])
    x, gy, y64, gx64 = operator_reference(complex_x, C, np.float64)
    op = TangentInterpolate()
    assert not list(op.parameters()) and not op.state_dict()

    def run():
        xd = T(x, dev).requires_grad_(True)
        y = op(xd, level)
        gx, = torch.autograd.grad(y, xd, T(gy, dev))
        return N_(y), N_(gx)
    (y, gx), (y2, gx2) = run(), run()
    assert y.shape == y64.shape == (162, C) and gx.shape == x.shape and y.dtype == x.dtype
    assert same_bits(y, y2) and same_bits(gx, gx2)
    for name, got, want, own in (('forward', y, y64, operator_reference(complex_x, C, np.float32)[2]),
                                 ('gradient', gx, gx64, operator_reference(complex_x, C, np.float32)[3])):
        err, gate = float(np.abs(got - want).max()), gate_of(want, own)
        print(f'\n{dtype} C={C} {name}: device against float64 {err:.3e}, gate {gate:.3e}')
        assert err <= gate


# ------------------------------------------------------------------ 4. a batch of two meshes; unreachable fine samples
BATCH_RADIUS = 0.9


@functools.lru_cache(maxsize=None)
def batch_parts():
    """[(pos, face, fine, coarse)]: the 162-vertex icosphere with 32 coarse samples, and sref.odd_mesh() -- a second component, a
    vertex in no face and vertex 47 on top of vertex 14 -- with every vertex fine and three coarse samples in the first component"""
    pos, face = sref.odd_mesh()
    return [ico_level(2, 'vertices'), (pos, face, np.arange(48, dtype=np.int64), np.array([2, 14, 25], dtype=np.int64))]


def test_batch_equals_the_single_meshes(dev):
    """with one radius for all: the default radius follows the largest cell of the whole batch, so it is given here"""
    from fieldconv_amd.transfer import interpolation_plan, tangent_transfer
    parts = batch_parts()
    singles = [interpolation_plan(T(p, dev), T(f, dev), T(s, dev), T(c, dev), radius=BATCH_RADIUS) for p, f, s, c in parts]
    pos, face, pos_ptr = gref.union([(p, f) for p, f, _, _ in parts])
    f_off, c_off = [0, 162], [0, 32]
    fine = np.concatenate([s + o for (_, _, s, _), o in zip(parts, pos_ptr[:-1])])
    coarse = np.concatenate([c + o for (_, _, _, c), o in zip(parts, f_off)])
    ptr, coarse_ptr = torch.tensor([0, 162, 210]), torch.tensor([0, 32, 35])
    both = interpolation_plan(T(pos, dev), T(face, dev), T(fine, dev), T(coarse, dev), radius=BATCH_RADIUS, pos_ptr=T(pos_ptr, dev), ptr=ptr,
                              coarse_ptr=coarse_ptr)
    assert (both.n_out, both.n_in) == (210, 35)
    rows, weight, phase = both.rows()
    each = [p.rows() for p in singles]
    want = torch.cat([r + torch.tensor([f_off[b], c_off[b]], device=dev) for b, (r, _, _) in enumerate(each)])
    assert torch.equal(rows, want)
    assert same_bits(N_(weight), N_(torch.cat([w for _, w, _ in each]))) and same_bits(N_(phase), N_(torch.cat([ph for _, _, ph in each])))
    # the odd mesh alone: its second component and the vertex in no face have no row; vertex 47 lies on coarse sample 14
    r1, w1, ph1 = (N_(t) for t in each[1])
    assert set(r1[:, 0].tolist()) == set(range(30)) | {47}
    own = np.nonzero(r1[:, 0] == 47)[0]
    assert r1[own[0], 1] == 1 and w1[own].tolist() == [1.0] + [0.0] * (len(own) - 1)
    x = T(tref.features(3, 4, True, 21).astype(np.complex64), dev)
    y = tangent_transfer(x, singles[1])
    assert bool((torch.view_as_real(y[30:47]) == 0).all()) and bool((y[:30].abs() > 0).all())
    got = N_(y[47])                                                                # the value of sample 14, turned into 47's frame
    assert np.abs(got - N_(x[1]) * ph1[own[0]]).max() <= 2.0 ** -22 * np.abs(N_(x[1])).max()


# ------------------------------------------------------------------ 5. CoarsenSamples
def test_coarsen_samples_carries_the_plan_only_when_asked(dev):
    from fieldconv_amd.transfer import interpolation_plan
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    pos, face = lref.icosphere(2)
    fine = SimpleNamespace(pos=T(pos, dev), face=T(face, dev))
    fine = ComputeLogXPort(0.7)(GeodesicSupportGraph(0.7, sample_n=96, random_start=False)(fine))
    plain, with_plan = CoarsenSamples(20, 1.2)(fine), CoarsenSamples(20, 1.2, interpolate_k=3)(fine)
    assert not hasattr(plain, 'interp') and (with_plan.interp.n_out, with_plan.interp.n_in) == (96, 20)
    for name in ('coarse', 'sample_idx', 'supp_edges', 'logMag', 'logAng', 'xp', 'w', 'cell'):
        assert same_bits(N_(getattr(plain, name)), N_(getattr(with_plan, name))), name
    assert plain.n_outside == with_plan.n_outside
    for name in ('pool', 'unpool'):
        for a, b in zip(getattr(plain, name).rows(), getattr(with_plan, name).rows()):
            assert same_bits(N_(a), N_(b))
    direct = interpolation_plan(fine.pos, fine.face, fine.sample_idx, plain.coarse)
    for a, b in zip(direct.rows(), with_plan.interp.rows()):
        assert same_bits(N_(a), N_(b))


# ------------------------------------------------------------------ 6. samples to every vertex
def test_vertex_interpolation_and_the_transform(dev):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.transfer import tangent_transfer, vertex_interpolation
    from fieldconv_amd.transforms import SamplesToVertices
    pos, face, _, samples = ico_level(2, 'vertices')
    data = SamplesToVertices(k=3)(SimpleNamespace(pos=T(pos, dev), face=T(face, dev), sample_idx=T(samples, dev)))
    plan = data.to_vertices
    assert (plan.n_out, plan.n_in) == (162, 32)
    for a, b in zip(plan.rows(), ico_plan(2, 'vertices', False)[0].rows()):       # the same construction, every vertex the fine level
        assert same_bits(N_(a), N_(b))
    rows, weight, phase = (N_(t) for t in plan.rows())
    first = np.searchsorted(rows[:, 0], samples)
    assert np.array_equal(rows[first, 1], np.arange(32)) and np.all(weight[first] == 1) and np.all(phase[first] == 1)
    logits = N_(tangent_transfer(torch.eye(32, device=dev), plan))                 # a one-hot labelling of the samples
    assert np.array_equal(logits[samples], np.eye(32, dtype=np.float32))           # the identity at the sampled vertices
    assert logits.min() >= 0 and logits.max() <= 1
    # a vertex's logits are its three weights themselves (w * 1 + 0): their float64 sum is 1 within 2 float32 ulps (test_interp_host)
    assert np.abs(logits.astype(np.float64).sum(1) - 1).max() <= 2 * 2.0 ** -23
    # a MeshBatch of two icospheres goes through the batched path: mesh for mesh the single plans (one radius for both)
    p3, f3, _, s3 = ico_level(3, 'vertices')
    batch = MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(p), face=torch.from_numpy(f)) for p, f in ((pos, face), (p3, f3))]).to(dev)
    batch.sample_idx = torch.cat((T(samples, dev), T(s3, dev) + 162))
    batch._set_ranges([32, 128], dev)
    both = SamplesToVertices(radius=0.9)(batch).to_vertices
    alone = [vertex_interpolation(T(p, dev), T(f, dev), T(s, dev), radius=0.9) for p, f, s in ((pos, face, samples), (p3, f3, s3))]
    assert (both.n_out, both.n_in) == (162 + 642, 32 + 128)
    want = torch.cat([a.rows()[0] + torch.tensor(o, device=dev) for a, o in zip(alone, ([0, 0], [162, 32]))])
    assert torch.equal(both.rows()[0], want)
    for i in (1, 2):
        assert same_bits(N_(both.rows()[i]), N_(torch.cat([a.rows()[i] for a in alone])))


# ------------------------------------------------------------------ 7. argument errors
def test_argument_errors_come_before_any_launch(dev):
    from fieldconv_amd.nn import TangentInterpolate
    from fieldconv_amd.transfer import interpolation_plan, knn_weights
    pos, face, fine, coarse = ico_level(2, 'vertices')
    p, f, s, c = T(pos, dev), T(face, dev), T(fine, dev), T(coarse, dev)
    for kw in (dict(k=0), dict(k=17), dict(power=3)):
        with pytest.raises(ValueError):
            interpolation_plan(p, f, s, c, **kw)
        with pytest.raises(ValueError):
            knn_weights(torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev),
                        torch.zeros(1, device=dev), **kw)
    with pytest.raises(ValueError):
        interpolation_plan(p, f, s, c.flip(0))
    level = SimpleNamespace(interp=ico_plan(2, 'vertices', False)[0])
    with pytest.raises(RuntimeError):
        TangentInterpolate()(torch.zeros(32, 4, dtype=torch.complex64), level)
