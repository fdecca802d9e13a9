"""The intrinsic gradient, divergence and Laplacian on the device (fieldconv_amd.diffops, csrc/fc_diffops.hip, transforms.GradientOperator)
against the numpy restatement tests/_diffops_ref.py, on the planted CSR of that module: rows of 0, 1, 2 (collinear), 2 (independent),
3, 63, 64, 65 and 129 slots among 70 samples with trailing empty rows, self rows, zero-weight neighbours, duplicates, shuffled.

Integer decisions (the two CSRs, valid, the zero pattern) are exact; no planted row lies within a factor 2 of the threshold, which
is asserted.  Coefficients: against the float64 restatement within max(4 x the float32 restatement's own error, 1e-6 x the largest
entry) -- cosf and sinf are the device library's.  Operators: given the DEVICE's coefficients, within 4 x the float32 restatement's
own error; in double within 1e-12 of the largest entry."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _diffops_ref as dref
import _geodesic_ref as gref

pytestmark = pytest.mark.gpu

DTYPES = {'float32': (torch.float32, torch.complex64, np.float32), 'float64': (torch.float64, torch.complex128, np.float64)}
CHANNELS = [1, 3, 48, 65]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev=torch.device('cuda:0')):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def same_bits(a, b):
    a, b = (torch.view_as_real(t) if t.is_complex() else t for t in (a, b))
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    as_int = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
    return bool((a.contiguous().view(as_int[a.element_size()]) == b.contiguous().view(as_int[b.element_size()])).all())


@functools.lru_cache(maxsize=None)
def restated(weighted=True):
    rows, mag, ang, w, n = dref.planted()
    return dref.Plan(rows, mag, ang, n, w if weighted else None)


def build_plan(weighted=True):
    from fieldconv_amd.functional import gradient_plan
    rows, mag, ang, w, n = dref.planted()
    return gradient_plan(T(rows), T(mag), T(ang), n, T(w).reshape(n, 1) if weighted else None)


@functools.lru_cache(maxsize=None)
def device_plan(weighted=True):
    return build_plan(weighted)


# ------------------------------------------------------------------ 1. the plan
@pytest.mark.parametrize('weighted', [True, False])
def test_plan_equals_the_restatement(dev, weighted):
    ref, plan = restated(weighted), device_plan(weighted)
    c64, d64, valid64, ratio = ref.coefficients(np.float64)
    c32, d32, valid32, _ = ref.coefficients(np.float32)
    finite = ratio[np.isfinite(ratio)]
    assert not ((finite > dref.RCOND / 2) & (finite < dref.RCOND * 2)).any()          # no row near the threshold: a flip cannot hide
    assert np.array_equal(valid32, valid64) and 0 < valid64.sum() < ref.n
    for name in ('rowptr', 'col', 'rowptr_t', 'col_t'):
        got = getattr(plan, name)
        assert got.dtype == torch.int32 and np.array_equal(N_(got), getattr(ref, name)), name
    assert plan.n == ref.n and plan.n_slots == len(ref.col)
    assert plan.valid.dtype == torch.uint8 and np.array_equal(N_(plan.valid), valid64)
    assert torch.is_tensor(plan.n_invalid) and plan.n_invalid.is_cuda and int(plan.n_invalid) == int((valid64 == 0).sum())
    coef, diag = N_(plan.coef), N_(plan.diag)
    assert coef.dtype == np.complex64 and diag.dtype == np.complex64
    assert np.array_equal(coef == 0, c64 == 0) and np.array_equal(diag == 0, d64 == 0)          # inactive slots, invalid and empty rows
    assert same_bits(plan.coef_t, plan.coef[T(ref.by_nbr)])
    for name, got, own, want in (('coef', coef, c32, c64), ('diag', diag, d32, d64)):
        err, gate = float(np.abs(got - want).max()), max(4 * float(np.abs(own - want).max()), 1e-6 * float(np.abs(want).max()))
        print(f'\n{name} weighted={weighted}: device against float64 {err:.3e}, gate {gate:.3e}, largest entry {np.abs(want).max():.3e}')
        assert err <= gate
    again = build_plan(weighted)
    for name in ('coef', 'coef_t', 'diag', 'valid', 'rowptr', 'col', 'rowptr_t', 'col_t'):
        assert same_bits(getattr(plan, name), getattr(again, name)), name
    if weighted:
        assert same_bits(plan.w, T(dref.planted()[3]))
        moved = plan.to('cuda:0')
        assert moved is plan
    else:
        assert plan.w is None


# ------------------------------------------------------------------ 2. the operators, forward and backward
@functools.lru_cache(maxsize=None)
def inputs(C):
    n = dref.N_PLANTED
    return dref.features(n, C, False, 10 + C), dref.features(n, C, True, 20 + C), dref.features(n, C, True, 30 + C), dref.features(n, C, False, 40 + C)


@functools.lru_cache(maxsize=None)
def reference(C, real, weighted):
    """the six results of the restatement in the arithmetic of `real`, with the device's coefficients"""
    ref, plan = restated(weighted), device_plan(weighted)
    k = dict(coef=N_(plan.coef), diag=N_(plan.diag))
    f, v, gy, gr = inputs(C)
    return dict(gradient=ref.gradient(f, real, **k), gradient_backward=ref.gradient_adjoint(gy, real, **k),
                divergence=ref.divergence(v, real, **k), divergence_backward=ref.divergence_adjoint(gr, real, **k),
                laplacian=ref.laplacian(f, real, **k), laplacian_backward=ref.laplacian_adjoint(gr, real, **k))


@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('weighted', [True, False])
def test_operators_and_their_gradients(dev, weighted, dtype, C):
    from fieldconv_amd.functional import laplacian, tangent_divergence, tangent_gradient
    rdt, cdt, real = DTYPES[dtype]
    plan = device_plan(weighted)
    f, v, gy, gr = inputs(C)

    def run():
        fd, vd = T(f, dev).to(rdt).requires_grad_(True), T(v, dev).to(cdt).requires_grad_(True)
        y, d, lap = tangent_gradient(fd, plan), tangent_divergence(vd, plan), laplacian(fd, plan)
        gf, = torch.autograd.grad(y, fd, T(gy, dev).to(cdt))
        gv, = torch.autograd.grad(d, vd, T(gr, dev).to(rdt))
        gl, = torch.autograd.grad(lap, fd, T(gr, dev).to(rdt))
        return dict(gradient=y.detach(), gradient_backward=gf, divergence=d.detach(), divergence_backward=gv, laplacian=lap.detach(),
                    laplacian_backward=gl)
    got, again = run(), run()
    want = reference(C, np.float64, weighted)
    valid = restated(weighted).coefficients(np.float64)[2]
    for name in want:
        complex_out = name in ('gradient', 'divergence_backward')
        assert got[name].dtype == (cdt if complex_out else rdt) and tuple(got[name].shape) == (dref.N_PLANTED, C), name
        assert same_bits(got[name], again[name]), name                       # no atomics, a fixed order: forward and backward
        err, top = float(np.abs(N_(got[name]) - want[name]).max()), float(np.abs(want[name]).max())
        gate = 4 * float(np.abs(reference(C, np.float32, weighted)[name] - want[name]).max()) if real == np.float32 else 1e-12 * top
        print(f'\n{name} weighted={weighted} {dtype} C={C}: device against float64 {err:.3e}, gate {gate:.3e}, largest entry {top:.3e}')
        assert err <= gate, name
    assert not N_(got['gradient'])[valid == 0].any()                          # an empty or invalid row is exactly zero


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_constants_give_exactly_zero(dev, dtype):
    from fieldconv_amd.functional import laplacian, tangent_gradient
    plan = device_plan()
    f = torch.full((dref.N_PLANTED, 5), 1.7, dtype=DTYPES[dtype][0], device=dev)
    assert not bool(torch.view_as_real(tangent_gradient(f, plan)).any()) and not bool(laplacian(f, plan).any())


def test_views_conjugates_and_frozen_inputs(dev):
    """a strided view and a lazily conjugated tensor are taken by value; an input that requires no gradient gets none"""
    from fieldconv_amd.functional import laplacian, tangent_divergence, tangent_gradient
    from fieldconv_amd.nn import TangentDivergence, TangentGradient
    plan = device_plan()
    f, v, _, _ = inputs(3)
    fd, vd = T(f, dev), T(v, dev)
    y, d = tangent_gradient(fd, plan), tangent_divergence(vd, plan)
    assert not y.requires_grad and not d.requires_grad and not laplacian(fd, plan).requires_grad
    wide = torch.zeros(dref.N_PLANTED, 6, device=dev)
    wide[:, ::2] = fd
    assert not wide[:, ::2].is_contiguous() and same_bits(tangent_gradient(wide[:, ::2], plan), y)
    assert same_bits(tangent_gradient(fd.t().contiguous().t(), plan), y)
    conj = vd.conj()
    assert conj.is_conj() and same_bits(tangent_divergence(conj, plan), tangent_divergence(conj.resolve_conj(), plan))
    assert not same_bits(tangent_divergence(conj, plan), d)
    neg = conj.imag                                                                              # a strided view with the lazy negative bit
    assert neg.is_neg() and same_bits(tangent_gradient(neg, plan), tangent_gradient(neg.resolve_neg().contiguous(), plan))
    assert same_bits(TangentGradient()(fd, plan), y) and same_bits(TangentDivergence()(vd, plan), d)
    frozen, live = T(f, dev), T(v, dev).requires_grad_(True)
    out = (tangent_divergence(live, plan) * laplacian(frozen, plan)).sum()
    out.backward()
    assert frozen.grad is None and live.grad is not None
    with pytest.raises(RuntimeError):
        tangent_gradient(fd.cpu(), plan)
    with pytest.raises(TypeError):
        tangent_gradient(vd, plan)
    with pytest.raises(ValueError):
        tangent_gradient(fd[:69], plan)


def test_adjoint_identity_on_the_device(dev):
    from fieldconv_amd.functional import tangent_divergence, tangent_gradient
    plan = device_plan()
    f, v, _, _ = inputs(3)
    fd, vd, w = T(f, dev).double(), T(v, dev).to(torch.complex128), plan.w.double()[:, None]
    g = tangent_gradient(fd, plan)
    lhs, rhs = float((w * (g.conj() * vd).real).sum()), -float((w * fd * tangent_divergence(vd, plan)).sum())
    # the adjoint subtracts diag, the FLOAT32 sum of a row's coefficients, where the exact transpose has their exact sum: the two sides
    # differ by that rounding and by nothing else
    query = torch.repeat_interleave(torch.arange(plan.n, device=dev), (plan.rowptr[1:] - plan.rowptr[:-1]).to(torch.int64))
    exact = torch.zeros(plan.n, dtype=torch.complex128, device=dev).index_add_(0, query, plan.coef.to(torch.complex128))
    slack = float((w * fd * ((plan.diag.to(torch.complex128) - exact).conj()[:, None] * vd).real).sum())
    scale = float((w * g.abs() * vd.abs()).sum())
    print(f'\nadjoint identity: {lhs:.12e} against {rhs:.12e}, of which diag\'s float32 rounding {slack:.3e}; scale {scale:.3e}')
    assert abs(lhs - rhs - slack) <= 1e-12 * scale


# ------------------------------------------------------------------ 3. end to end: a lattice through the transforms
ALPHA, BETA, GAMMA = 0.75, -1.25, 0.5          # dyadic, like the lattice's coordinates: the affine function is exact in float32
EPSILON = 0.3


def chain(data):
    from fieldconv_amd.transforms import ComputeLogXPort, GeodesicSupportGraph, GradientOperator
    return GradientOperator()(ComputeLogXPort(EPSILON)(GeodesicSupportGraph(EPSILON)(data)))


def affine(pos):
    return (ALPHA * pos[:, 0] + BETA * pos[:, 1] + GAMMA)[:, None].contiguous()


@functools.lru_cache(maxsize=None)
def lattices():
    meshes = [gref.lattice(9, 9), gref.lattice(7, 8)]
    return meshes, [chain(SimpleNamespace(pos=T(p), face=T(f))) for p, f in meshes]


def test_lattice_gradient_of_an_affine_function(dev):
    from fieldconv_amd.functional import tangent_gradient
    from fieldconv_amd.transforms import vertex_frames
    data = lattices()[1][0]
    plan = data.grad_plan
    assert plan.n == 81 and data.sample_idx.tolist() == list(range(81))
    valid = plan.valid.bool()
    assert int(valid.sum()) >= 49
    g = tangent_gradient(affine(data.pos), plan)[:, 0]
    _, e1, e2 = vertex_frames(data.pos, data.face)
    want = torch.complex(ALPHA * e1[:, 0] + BETA * e1[:, 1], ALPHA * e2[:, 0] + BETA * e2[:, 1])
    err = float((g - want).abs()[valid].max())
    print(f'\nlattice: {int(valid.sum())} valid rows of 81, |G f - (alpha, beta)| at most {err:.3e} of {abs(complex(ALPHA, BETA)):.3f}')
    assert err <= 1e-5 * abs(complex(ALPHA, BETA))
    assert not bool(torch.view_as_real(g[~valid]).any())


def test_batch_equals_the_single_meshes(dev):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.functional import laplacian, tangent_gradient
    meshes, singles = lattices()
    batch = chain(MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(p), face=torch.from_numpy(f)) for p, f in meshes]).to(dev))
    assert batch.ptr.tolist() == [0, 81, 137] and batch.grad_plan.n == 137
    f = affine(batch.pos) * batch.pos[:, :1]          # not affine: a Laplacian that is not zero
    g, lap = tangent_gradient(f, batch.grad_plan), laplacian(f, batch.grad_plan)
    for b, single in enumerate(singles):
        lo, hi = batch.ptr.tolist()[b:b + 2]
        own = f[lo:hi].contiguous()
        assert same_bits(batch.grad_plan.valid[lo:hi], single.grad_plan.valid) and same_bits(batch.grad_plan.diag[lo:hi], single.grad_plan.diag)
        assert same_bits(g[lo:hi], tangent_gradient(own, single.grad_plan)) and same_bits(lap[lo:hi], laplacian(own, single.grad_plan))


def test_laplacian_replays_inside_a_step_graph(dev):
    from fieldconv_amd.functional import laplacian
    from fieldconv_amd.utils import StepGraph
    plan = device_plan()
    f, _, _, gr = inputs(48)
    fd, gd = T(f, dev).requires_grad_(True), T(gr, dev)

    def step():
        lap = laplacian(fd, plan)
        return (lap.detach(),) + torch.autograd.grad(lap, fd, gd)
    eager = [t.clone() for t in step()]
    graphed = StepGraph(step)
    for _ in range(2):
        assert all(same_bits(a, b) for a, b in zip(graphed.replay(), eager))
