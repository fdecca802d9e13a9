"""Host-side checks of the intrinsic gradient, divergence and Laplacian (fieldconv_amd.diffops, csrc/fc_diffops.hip): the float64
numpy restatement tests/_diffops_ref.py against what the operators must satisfy on meshes whose log map is known exactly --
exactness on affine functions, zero on constants, the adjoint identity, symmetry and sign of the Laplacian, gauge equivariance,
convergence on the sphere -- and the C ABI surface, the argument checks and the exports, none of which needs a device."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _diffops_ref as dref
import _geodesic_ref as gref
import _logmap_ref as lref
from conftest import ROOT

F64 = np.float64
SYMBOLS = {'fc_gradient_coefficients', 'fc_gradient_apply', 'fc_gradient_adjoint'}
H = 0.125


def lattice_plan(theta=None, weighted=True):
    pos, _ = gref.lattice(9, 9, H)
    rows, mag, ang = dref.planar_rows(pos, 2.5 * H, theta)
    w = np.random.default_rng(3).uniform(0.5, 2.0, len(pos)) if weighted else None
    return pos.astype(F64), dref.Plan64(rows, mag, ang, len(pos), w)


def w_dot(w, a, b):
    """the W inner product of two fields, real or complex: sum_a w_a Re(conj(a) b) over samples and channels"""
    return float((w[:, None] * (np.conj(a) * b).real).sum())


# ------------------------------------------------------------------ 1. exactness, constants
def test_gradient_of_an_affine_function_is_exact_on_a_lattice():
    pos, plan = lattice_plan()
    coef, diag, valid, ratio = plan.coefficients(F64)
    assert valid.all() and ratio.min() > 0.01                      # corners and borders included: every ball spans the plane
    assert np.abs(diag - np.add.reduceat(coef, plan.rowptr[:-1])).max() <= 1e-9 * np.abs(coef).max()
    for alpha, beta, gamma in ((0.75, -1.25, 0.5), (0.0, 1.0, 0.0), (-2.0, 0.0, 3.0)):
        f = (alpha * pos[:, 0] + beta * pos[:, 1] + gamma)[:, None]
        g = plan.gradient(f, F64)
        assert np.abs(g - (alpha + 1j * beta)).max() <= 1e-12 * max(abs(alpha), abs(beta))


def test_constants_give_exactly_zero():
    pos, plan = lattice_plan()
    f = np.full((len(pos), 3), 1.7)
    assert not plan.gradient(f, F64).any() and not plan.laplacian(f, F64).any()
    assert not plan.gradient(f.astype(np.float32), np.float32).any() and not plan.laplacian(f.astype(np.float32), np.float32).any()


# ------------------------------------------------------------------ 2. adjoint identity, the Laplacian's symmetry and sign
def test_divergence_is_the_negative_adjoint_and_the_laplacian_is_symmetric_negative_semidefinite():
    pos, plan = lattice_plan()
    n, w = len(pos), plan.w
    f, u = dref.features(n, 4, False, 1).astype(F64), dref.features(n, 4, False, 2).astype(F64)
    v = dref.features(n, 4, True, 3).astype(np.complex128)
    gf = plan.gradient(f, F64)
    lhs, rhs = w_dot(w, gf, v), -w_dot(w, f, plan.divergence(v, F64))
    assert abs(lhs - rhs) <= 1e-12 * float((w[:, None] * np.abs(gf) * np.abs(v)).sum())
    lf, lu = plan.laplacian(f, F64), plan.laplacian(u, F64)
    energy = w_dot(w, gf, gf)
    assert w_dot(w, f, lf) <= 0 and abs(w_dot(w, f, lf) + energy) <= 1e-12 * energy          # -Dirichlet energy
    assert abs(w_dot(w, u, lf) - w_dot(w, lu, f)) <= 1e-12 * float((w[:, None] * np.abs(u) * np.abs(lf)).sum())
    # the adjoints the autograd nodes run are the transposes of the forward maps
    g = dref.features(n, 4, False, 4).astype(F64)
    assert abs(float((g * plan.divergence(v, F64)).sum()) - float((np.conj(plan.divergence_adjoint(g, F64)) * v).real.sum())) <= 1e-9
    assert abs(float((np.conj(v) * gf).real.sum()) - float((plan.gradient_adjoint(v, F64) * f).sum())) <= 1e-9
    assert abs(float((g * lf).sum()) - float((plan.laplacian_adjoint(g, F64) * f).sum())) <= 1e-7


def test_unweighted_plan_uses_unit_weights():
    pos, plan = lattice_plan(weighted=False)
    f, v = dref.features(len(pos), 2, False, 5).astype(F64), dref.features(len(pos), 2, True, 6).astype(np.complex128)
    lhs, rhs = float((np.conj(plan.gradient(f, F64)) * v).real.sum()), -float((f * plan.divergence(v, F64)).sum())
    assert abs(lhs - rhs) <= 1e-12 * float((np.abs(plan.gradient(f, F64)) * np.abs(v)).sum())


# ------------------------------------------------------------------ 3. gauge
def test_regauging_the_frames():
    theta = np.random.default_rng(7).uniform(-np.pi, np.pi, 81)
    (pos, plan), (_, turned) = lattice_plan(), lattice_plan(theta)
    rot = np.exp(-1j * theta)[:, None]
    f, v = dref.features(81, 3, False, 8).astype(F64), dref.features(81, 3, True, 9).astype(np.complex128)
    g = plan.gradient(f, F64)
    assert np.abs(turned.gradient(f, F64) - rot * g).max() <= 1e-12 * np.abs(g).max()
    d = plan.divergence(v, F64)
    assert np.abs(turned.divergence(rot * v, F64) - d).max() <= 1e-12 * np.abs(d).max()
    lap = plan.laplacian(f, F64)
    assert np.abs(turned.laplacian(f, F64) - lap).max() <= 1e-12 * np.abs(lap).max()


# ------------------------------------------------------------------ 4. degenerate rows
def test_planted_rows_are_away_from_the_threshold_and_degenerate_rows_are_zero():
    rows, mag, ang, w, n = dref.planted()
    plan = dref.Plan(rows, mag, ang, n, w)
    lengths = np.diff(plan.rowptr)
    assert [int(lengths[a]) for a in sorted(dref.ROW_LENGTHS)] == list(dref.ROW_LENGTHS.values()) and not lengths[50:].any()
    for real in (np.float32, F64):
        coef, diag, valid, ratio = plan.coefficients(real)
        assert valid[:9].tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 1] and valid[9:50].all() and not valid[50:].any()
        assert not coef[plan.rowptr[0]:plan.rowptr[3]].any() and not diag[:3].any() and not diag[50:].any()
        inactive = (plan.col == np.repeat(np.arange(n), lengths)) | np.isin(plan.col, dref.ZERO_WEIGHT)
        assert inactive.sum() >= 2 * 45 and not coef[inactive].any() and (coef[~inactive & (valid[np.repeat(np.arange(n), lengths)] == 1)] != 0).all()
    ratio = plan.coefficients(F64)[3]
    finite = ratio[np.isfinite(ratio)]
    assert not ((finite > dref.RCOND / 2) & (finite < dref.RCOND * 2)).any()


# ------------------------------------------------------------------ 5. accuracy on the sphere
def test_accuracy_improves_with_resolution_on_the_icosphere(capsys):
    """grad z against the projection of e_z into the tangent plane, in the vertex frame; every vertex a sample, the closed-form
    log map of the sphere, balls of 2.5 mean edge lengths.  The figures are printed; the gate is the order of the two means.
    A linear fit over a ball of radius r sees sin(d) / d in place of 1 at distance d, so the error is of order r^2 / 6.
    Measured: 162 vertices (18.1 rows per query) mean 5.23e-02 worst 9.95e-02; 642 vertices (19.2) mean 1.89e-02 worst 4.73e-02."""
    means = []
    for sub in (2, 3):
        pos, face = lref.icosphere(sub)
        rows, mag, ang = dref.sphere_rows(pos, 2.5 * dref.mean_edge_length(pos, face))
        plan = dref.Plan64(rows, mag, ang, len(pos))
        nrm, e1, e2 = dref.sphere_frames(pos)
        assert plan.coefficients(F64)[2].all()
        got = plan.gradient(nrm[:, 2:3], F64)[:, 0]
        want = e1[:, 2] + 1j * e2[:, 2]          # e_z - (e_z . n) n in (e1, e2): the normal part has no component there
        err = np.abs(got - want)
        means.append(float(err.mean()))
        with capsys.disabled():
            print(f'\nicosphere {len(pos)} vertices, {len(rows) / len(pos):.1f} rows per query: |grad z - P e_z| mean {err.mean():.3e} worst {err.max():.3e}')
    assert means[1] < means[0]


# ------------------------------------------------------------------ 6. ABI, checks, exports
def test_abi_surface_and_argument_checks():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES) and 'fc_diffops.hip' in build.SOURCES
    assert [len(_lib.SIGNATURES[s][1]) for s in sorted(SYMBOLS)] == [13, 10, 12]
    lib = _lib.load()
    assert lib.fc_abi_version() == 11
    one = ctypes.c_void_p(16)          # never dereferenced: every call below returns before a launch
    assert lib.fc_gradient_coefficients(None, None, None, None, None, 1e-4, 0, 0, None, None, None, None) == 0
    assert lib.fc_gradient_apply(None, None, None, None, 0, 0, 4, 0, None, None) == 0
    assert lib.fc_gradient_adjoint(None, None, None, None, None, None, None, 0, 0, 4, 1, None, None) == 0
    for rcond in (-1.0, 2.0, float('nan')):
        assert lib.fc_gradient_coefficients(one, one, one, one, None, rcond, 4, 4, one, one, one, None) == -1
    assert lib.fc_gradient_coefficients(None, one, one, one, None, 1e-4, 4, 4, one, one, one, None) == -1
    for n, slots, C, dt in ((-1, 0, 4, 0), (4, -1, 4, 0), (4, 4, 0, 0), (4, 4, 4, 2)):
        assert lib.fc_gradient_apply(one, one, one, one, n, slots, C, dt, one, None) == -1
        assert lib.fc_gradient_adjoint(one, one, one, one, one, None, None, n, slots, C, dt, one, None) == -1
    assert lib.fc_gradient_apply(None, one, one, one, 4, 4, 4, 0, one, None) == -1
    assert lib.fc_gradient_adjoint(one, one, one, one, None, None, None, 4, 4, 4, 0, one, None) == -1


def test_python_checks_raise_before_any_launch():
    from fieldconv_amd import diffops
    rows = torch.tensor([[0, 1], [1, 0]])
    mag, ang = torch.ones(2), torch.zeros(2)
    bad = [dict(supp_edges=rows.to(torch.int32)), dict(supp_edges=rows[:, :1]), dict(logMag=mag.double()), dict(logAng=ang[:1]),
           dict(n=1), dict(n=-1), dict(n=2.5), dict(w=torch.ones(3)), dict(w=torch.ones(2).double()), dict(rcond=-1), dict(rcond='x'),
           dict(rcond=float('nan'))]
    for change in bad:
        args = dict(supp_edges=rows, logMag=mag, logAng=ang, n=2, w=None, rcond=1e-4)
        args.update(change)
        with pytest.raises(ValueError):
            diffops.gradient_plan(**args)
    plan = diffops.GradientPlan(2, 2, *[None] * 9, None, 1e-4, torch.device('cuda', 0))
    with pytest.raises(TypeError):
        diffops.tangent_gradient(torch.zeros(2, 3, dtype=torch.complex64), plan)          # complex input: not a scalar field
    with pytest.raises(TypeError):
        diffops.tangent_divergence(torch.zeros(2, 3), plan)
    with pytest.raises(TypeError):
        diffops.laplacian(torch.zeros(2, 3, dtype=torch.float16), plan)
    with pytest.raises(RuntimeError):
        diffops.tangent_gradient(torch.zeros(2, 3), plan)                                 # no CPU path
    with pytest.raises(ValueError):
        diffops.tangent_gradient(torch.zeros(2, 3), object())
    with pytest.raises(ValueError):
        diffops.tangent_gradient(torch.zeros(6), plan)


def test_exports_and_parameter_free_modules():
    from fieldconv_amd import diffops, functional, nn, transforms
    for name in ('GradientPlan', 'gradient_plan', 'tangent_gradient', 'tangent_divergence', 'laplacian'):
        assert getattr(functional, name) is getattr(diffops, name)
    assert {'TangentGradient', 'TangentDivergence'} <= set(nn.__all__) and 'GradientOperator' in transforms.__all__
    for cls in (nn.TangentGradient, nn.TangentDivergence):
        assert not cls().state_dict() and not list(cls().parameters())
    assert repr(transforms.GradientOperator()) == 'GradientOperator(rcond=0.0001)'
    with pytest.raises(ValueError):
        transforms.GradientOperator(rcond=-1)
    with pytest.raises(ValueError):
        transforms.GradientOperator()(type('D', (), {})())
