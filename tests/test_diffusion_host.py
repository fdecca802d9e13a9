"""Heat diffusion on the host: the numpy restatement tests/_diffusion_ref.py against linear algebra.  What the device tests
(tests/test_gpu_diffusion.py) compare the kernels with is checked here for being the right thing: S Hermitian and positive
semidefinite whatever the rows are, the recurrence reaching the dense solve, the implicit gradients against central
differences, gauge equivariance, the two limits of t, and -- recorded, not gated -- the Laplacian of the icosphere."""
import numpy as np

import _diffops_ref as gref
import _diffusion_ref as dref
import _logmap_ref as lref

F64 = np.float64


def planted_plan():
    rows, xp, mag, w, n = dref.planted()
    return dref.Plan(rows, xp, mag, n, w)


def small_system(seed=3, n=40, connected=True):
    """a planted system of 40 rows: a ring plus random chords, symmetric pairs with conjugate transports, positive masses"""
    rng = np.random.RandomState(seed)
    pairs = [(i, (i + 1) % n) for i in range(n)] + [(int(a), int(b)) for a, b in rng.randint(0, n, (30, 2)) if a != b]
    rows, xp = [], []
    for a, b in pairs:
        u = np.exp(1j * rng.uniform(-np.pi, np.pi))
        rows += [(a, b), (b, a)]
        xp += [u, np.conj(u)]
    rows, xp = np.array(rows, dtype=np.int64), np.array(xp).astype(np.complex64)
    mag = np.repeat(rng.uniform(0.1, 0.3, len(pairs)), 2).astype(np.float32)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    return dref.Plan(rows, xp, mag, n, w, h=0.02)


def test_stiffness_is_hermitian_and_positive_semidefinite():
    plan = planted_plan()
    rows, xp, mag, w, n = dref.planted()
    lengths = np.diff(plan.rowptr)
    assert [int(lengths[i]) for i in range(5)] == [0, 1, 64, 65, 130] and w[7] == 0 and (rows[:, 0] == rows[:, 1]).any()
    assert 0 < (~plan.active).sum() < len(rows)
    coef, g, diag, diag_real = plan.values(np.float32)
    # to the last bit of the stored entries: every entry (i, j, v) has its partner (j, i, conj(v))
    own = sorted((i, int(plan.col[k]), float(coef[k].real), float(coef[k].imag)) for i in range(n) for k in range(plan.rowptr[i], plan.rowptr[i + 1]))
    partner = sorted((int(plan.col[k]), i, float(coef[k].real), -float(coef[k].imag)) for i in range(n) for k in range(plan.rowptr[i], plan.rowptr[i + 1]))
    assert own == partner
    inactive = ~plan.active[np.where(plan.edge < 0, -plan.edge - 1, plan.edge)]
    assert np.array_equal(coef == 0, inactive) and np.array_equal(g == 0, inactive)
    assert diag[0] == 0 and diag_real[0] == 0 and diag[6] == 0          # the empty row; the self row contributes nothing
    for complex_x in (True, False):
        S = plan.dense(complex_x)
        assert np.abs(S - S.conj().T).max() <= 1e-15 * np.abs(S).max()
        low = np.linalg.eigvalsh((S + S.conj().T) / 2).min()
        print(f'\nS {"complex" if complex_x else "real"}: smallest eigenvalue {low:.3e} of {np.abs(S).max():.3e}')
        assert low >= -1e-6 * np.abs(S).max()          # (the stored diagonal is a float32 sum)
    S64 = plan.dense(True, plan.values(F64))
    assert np.linalg.eigvalsh(S64).min() >= -1e-13 * np.abs(S64).max()


def test_real_stiffness_annihilates_constants():
    plan = planted_plan()
    ones = np.ones((plan.n, 2))
    out = dref.stiffness(plan, ones, F64, plan.values(F64))
    assert np.abs(out).max() <= 1e-13 * np.abs(plan.values(F64)[3]).max()
    assert np.abs(dref.laplacian(plan, ones, F64, plan.values(F64))).max() <= 1e-10


def test_recurrence_reaches_the_dense_solve():
    plan = small_system()
    vals = plan.values(F64)
    for complex_x in (True, False):
        x = dref.features(plan.n, 3, complex_x, 5).astype(np.complex128 if complex_x else F64)
        t = np.array([0.05, 0.5, 2.0])
        y = dref.heat_diffuse(plan, x, t, F64, plan.n, values=vals)
        want = dref.dense_solve(plan, x, t, vals)
        err = np.abs(y - want).max() / np.abs(want).max()
        print(f'\niters = n = {plan.n}, complex={complex_x}: against np.linalg.solve {err:.3e}')
        assert err <= 1e-10


def test_implicit_gradients_match_central_differences():
    plan = small_system(seed=4)
    vals = plan.values(F64)
    x = dref.features(plan.n, 2, True, 6).astype(np.complex128)
    gy = dref.features(plan.n, 2, True, 7).astype(np.complex128)
    t = np.array([0.3, 1.1])
    gx, gt = dref.heat_diffuse_backward(plan, x, t, gy, F64, plan.n, values=vals)
    loss = lambda xx, tt: float(np.sum((np.conj(gy) * dref.dense_solve(plan, xx, tt, vals)).real))
    eps = 1e-6
    for c in range(2):
        dt = np.zeros(2)
        dt[c] = eps
        fd = (loss(x, t + dt) - loss(x, t - dt)) / (2 * eps)
        assert abs(fd - gt[c]) <= 1e-6 * max(1.0, abs(gt[c])), (fd, gt[c])
    rng = np.random.RandomState(0)
    for _ in range(4):
        i, c = rng.randint(plan.n), rng.randint(2)
        for unit, part in ((1.0, np.real), (1j, np.imag)):
            dx = np.zeros_like(x)
            dx[i, c] = eps * unit
            fd = (loss(x + dx, t) - loss(x - dx, t)) / (2 * eps)
            assert abs(fd - part(gx[i, c])) <= 1e-6 * max(1.0, abs(gx[i, c]))


def test_gauge_equivariance():
    base = small_system(seed=8)
    rng = np.random.RandomState(1)
    theta = rng.uniform(-np.pi, np.pi, base.n)
    a, b = base.rows[:, 0], base.rows[:, 1]
    # in double, so that the re-gauged transports carry no float32 rounding of their own
    plan = dref.Plan(base.rows, base.xp.astype(np.complex128), base.mag, base.n, base.w, base.h)
    turned = dref.Plan(base.rows, base.xp.astype(np.complex128) * np.exp(-1j * (theta[b] - theta[a])), base.mag, base.n, base.w, base.h)
    x = dref.features(base.n, 2, True, 9).astype(np.complex128)
    t = np.array([0.2, 0.9])
    y = dref.heat_diffuse(plan, x, t, F64, 16, values=plan.values(F64))
    y2 = dref.heat_diffuse(turned, np.exp(-1j * theta)[:, None] * x, t, F64, 16, values=turned.values(F64))
    assert np.abs(y2 - np.exp(-1j * theta)[:, None] * y).max() <= 1e-12 * np.abs(y).max()


def test_limits_of_the_diffusion_time():
    plan = small_system(seed=10)
    vals = plan.values(F64)
    x = dref.features(plan.n, 2, False, 11).astype(F64)
    y0 = dref.heat_diffuse(plan, x, np.zeros(2), F64, 8, values=vals)
    assert np.array_equal(y0, x)
    y = dref.heat_diffuse(plan, x, np.array([1e7, 1e7]), F64, plan.n, values=vals)
    w = plan.w.astype(F64)
    mean = (w[:, None] * x).sum(0) / w.sum()
    print(f'\nt = 1e7: distance from the w-mean {np.abs(y - mean).max():.3e}')
    assert np.abs(y - mean).max() <= 1e-4 * np.abs(x).max()


def test_icosphere_laplacian_error_is_recorded():
    """L z against -2 z (z a coordinate function: an eigenfunction of the sphere's Laplacian) on the 642-vertex icosphere with the
    closed-form log map.  Recorded, not gated: the point-cloud heat kernel converges slowly and is biased at this h."""
    pos, face = lref.icosphere(3)
    pos = np.asarray(pos, dtype=np.float64)
    radius = 2.5 * gref.mean_edge_length(pos, np.asarray(face))
    rows, mag, ang = gref.sphere_rows(pos, radius)[:3]
    area = 4 * np.pi / len(pos)
    plan = dref.Plan(np.asarray(rows, dtype=np.int64), np.ones(len(rows), dtype=np.complex64), np.asarray(mag, dtype=np.float32), len(pos),
                     np.full(len(pos), area, dtype=np.float32))
    z = pos[:, 2:3]
    lz = dref.laplacian(plan, z, F64, plan.values(F64))
    err = np.abs(lz + 2 * z).max()
    print(f'\nicosphere 642: h = {plan.h:.4e}, |L z + 2 z| at most {err:.3e} (|2 z| at most 2)')
    assert np.isfinite(err)
