"""Heat diffusion on the device (fieldconv_amd.diffusion, csrc/fc_diffusion.hip, nn.TangentDiffusion, transforms.DiffusionOperator)
against the numpy restatement tests/_diffusion_ref.py on its planted plan: 67 samples whose matrix rows hold 0, 1, 64, 65 and 130
entries, with duplicates, a self row, a zero-weight sample, one-directional and inactive rows.

Integer decisions (the merged CSR, the active mask, the zero pattern) are exact.  Coefficients: against the float64 restatement
within max(4 x the float32 restatement's own error, 1e-6 x the largest entry) -- expf is the device library's.  Operators and
solves: given the DEVICE's coefficients, within max(4 x the float32 restatement's own error, 1e-6 x the largest entry) in single
precision and 1e-10 x the largest entry in double.  The invariances (runs, C, batch, where p lives) are exact."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _diffusion_ref as dref
import _geodesic_ref as gref

pytestmark = pytest.mark.gpu

DTYPES = {'float32': (torch.float32, np.float32, False), 'float64': (torch.float64, np.float64, False),
          'complex64': (torch.complex64, np.float32, True), 'complex128': (torch.complex128, np.float64, True)}
CHANNELS = [1, 5, 48]
ITERS = [1, 2, 16]


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


def gate(got, want, own, real, what):
    err, top = float(np.abs(got - want).max()), float(np.abs(want).max())
    if real == np.float32:
        own_err = float(np.abs(own - want).max())
        assert own_err <= 1e-3 * top, f'{what}: the float32 restatement itself is off by {own_err:.3e} of {top:.3e}: the gate is vacuous'
        bound = max(4 * own_err, 1e-6 * top)
    else:
        bound = 1e-10 * top
    print(f'\n{what}: device against float64 {err:.3e}, gate {bound:.3e}, largest entry {top:.3e}')
    assert err <= bound, what


@functools.lru_cache(maxsize=None)
def restated():
    rows, xp, mag, w, n = dref.planted()
    return dref.Plan(rows, xp, mag, n, w)


def build_plan(weighted=True, h=None):
    from fieldconv_amd.functional import diffusion_plan
    rows, xp, mag, w, n = dref.planted()
    return diffusion_plan(T(rows), T(xp), T(mag), n, T(w).reshape(n, 1) if weighted else None, h)


@functools.lru_cache(maxsize=None)
def device_plan():
    return build_plan()


@functools.lru_cache(maxsize=None)
def device_values():
    plan = device_plan()
    return N_(plan.coef), N_(plan.coef_real), N_(plan.diag), N_(plan.diag_real)


# ------------------------------------------------------------------ 1. the plan
def test_plan_equals_the_restatement(dev):
    from fieldconv_amd.diffusion import LDS_ROWS, DiffusionPlan
    from fieldconv_amd import _lib
    ref, plan = restated(), device_plan()
    assert isinstance(plan, DiffusionPlan) and plan.n == ref.n and plan.n_entries == len(ref.col) == 2 * len(ref.rows)
    assert plan.h == ref.h
    assert all(v == _lib.load().fc_diffusion_lds_rows() for v in LDS_ROWS.values()) and set(LDS_ROWS) == {d[0] for d in DTYPES.values()}
    for name in ('rowptr', 'col', 'edge'):
        got = getattr(plan, name)
        assert got.dtype == torch.int32 and np.array_equal(N_(got), getattr(ref, name)), name
    want, own, got = ref.values(np.float64), ref.values(np.float32), device_values()
    inactive = ~ref.active[np.where(ref.edge < 0, -ref.edge - 1, ref.edge)]
    assert got[0].dtype == np.complex64 and all(g.dtype == np.float32 for g in got[1:])
    assert np.array_equal(got[0] == 0, inactive) and np.array_equal(got[1] == 0, inactive)          # the active mask, the zero pattern
    assert np.array_equal(got[2] == 0, want[2] == 0) and np.array_equal(got[3] == 0, want[3] == 0)
    for name, g, o, w_ in zip(('coef', 'coef_real', 'diag', 'diag_real'), got, own, want):
        gate(g, w_, o, np.float32, name)
    # Hermitian to the last bit of the stored entries
    k = np.arange(plan.n_entries)
    row = np.repeat(np.arange(ref.n), np.diff(ref.rowptr))
    own_e = sorted(zip(row.tolist(), ref.col.tolist(), got[0].real.tolist(), got[0].imag.tolist()))
    partner = sorted(zip(ref.col.tolist(), row.tolist(), got[0].real.tolist(), (-got[0].imag).tolist()))
    assert own_e == partner and len(k) == len(own_e)
    again = build_plan()
    for name in ('coef', 'coef_real', 'diag', 'diag_real', 'rowptr', 'col', 'edge'):
        assert same_bits(getattr(plan, name), getattr(again, name)), name
    assert plan.to('cuda:0') is plan and build_plan(False).w is None
    fixed = build_plan(h=0.01)
    assert fixed.h == 0.01 and not same_bits(fixed.coef, plan.coef)


# ------------------------------------------------------------------ 2. Laplacian and solve against the restatement
@functools.lru_cache(maxsize=None)
def inputs(C, complex_x):
    n = dref.N_PLANTED
    return dref.features(n, C, complex_x, 10 + C), dref.features(n, C, complex_x, 20 + C), dref.times(C)


@functools.lru_cache(maxsize=None)
def reference(C, complex_x, real, iters):
    ref, vals = restated(), device_values()
    x, gy, t = inputs(C, complex_x)
    out = dict(laplacian=dref.laplacian(ref, x, real, vals), laplacian_backward=dref.laplacian_adjoint(ref, gy, real, vals),
               y=dref.heat_diffuse(ref, x, t, real, iters, values=vals))
    out['gx'], out['gt'] = dref.heat_diffuse_backward(ref, x, t, gy, real, iters, values=vals)
    return out


@pytest.mark.parametrize('iters', ITERS)
@pytest.mark.parametrize('C', CHANNELS)
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_operators_and_their_gradients(dev, dtype, C, iters):
    from fieldconv_amd.functional import connection_laplacian, heat_diffuse
    tdt, real, complex_x = DTYPES[dtype]
    rdt = torch.float64 if real == np.float64 else torch.float32
    plan = device_plan()
    x, gy, t = inputs(C, complex_x)

    def run():
        xd, td, gd = T(x, dev).to(tdt).requires_grad_(True), T(t, dev).to(rdt).requires_grad_(True), T(gy, dev).to(tdt)
        lap = connection_laplacian(xd, plan)
        gl, = torch.autograd.grad(lap, xd, gd)
        y = heat_diffuse(xd, td, plan, iters=iters)
        gx, gt = torch.autograd.grad(y, [xd, td], gd)
        return dict(laplacian=lap.detach(), laplacian_backward=gl, y=y.detach(), gx=gx, gt=gt)
    got, again = run(), run()
    want, own = reference(C, complex_x, np.float64, iters), reference(C, complex_x, np.float32, iters)
    for name in want:
        assert got[name].dtype == (rdt if name == 'gt' else tdt) and tuple(got[name].shape) == ((C,) if name == 'gt' else (dref.N_PLANTED, C))
        assert same_bits(got[name], again[name]), name          # two runs give the same bits
        gate(N_(got[name]), want[name], own[name], real, f'{name} {dtype} C={C} iters={iters}')
    if C > 1:          # t = 0: y has x's bits, and its time receives the gradient of the exact solve at t = 0 (r = 0 adds nothing)
        assert same_bits(got['y'][:, 1].contiguous(), T(x, dev).to(tdt)[:, 1].contiguous())


# ------------------------------------------------------------------ 3. exact invariances
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_a_channel_does_not_depend_on_its_neighbours_or_on_where_p_lives(dev, dtype):
    from fieldconv_amd.functional import heat_diffuse
    tdt, real, complex_x = DTYPES[dtype]
    rdt = torch.float64 if real == np.float64 else torch.float32
    plan = device_plan()
    x, gy, t = inputs(48, complex_x)
    xd, td, gd = T(x, dev).to(tdt), T(t, dev).to(rdt), T(gy, dev).to(tdt)

    def both(xs, ts, gs, **kw):
        xs, ts = xs.clone().requires_grad_(True), ts.clone().requires_grad_(True)
        y, res = heat_diffuse(xs, ts, plan, iters=16, return_residual=True, **kw)
        return (y.detach(), res) + torch.autograd.grad(y, [xs, ts], gs)
    wide = both(xd, td, gd)
    alone = both(xd[:, 3:4].contiguous(), td[3:4].contiguous(), gd[:, 3:4].contiguous())
    assert wide[1].shape == (1, 48) and not wide[1].requires_grad
    for a, b in zip(wide, alone):
        assert same_bits((a[:, 3:4] if a.dim() == 2 else a[3:4]).contiguous(), b)
    forced = both(xd, td, gd, _state='workspace')
    assert all(same_bits(a, b) for a, b in zip(wide, forced))


@pytest.mark.parametrize('dtype', ['complex64', 'float64'])
def test_a_mesh_alone_equals_the_mesh_inside_a_batch(dev, dtype):
    """three meshes side by side, the middle one empty: the planted plan twice, rows of the second shifted by 67"""
    from fieldconv_amd.functional import diffusion_plan, heat_diffuse
    tdt, real, complex_x = DTYPES[dtype]
    rdt = torch.float64 if real == np.float64 else torch.float32
    rows, xp, mag, w, n = dref.planted()
    single = device_plan()
    batch = diffusion_plan(T(np.concatenate([rows, rows + n])), T(np.concatenate([xp, xp])), T(np.concatenate([mag, mag])), 2 * n,
                           T(np.concatenate([w, w])), single.h)
    assert same_bits(batch.coef[:single.n_entries], single.coef) and same_bits(batch.diag[n:], single.diag)
    x, gy, t = inputs(5, complex_x)
    x2, g2 = T(np.concatenate([x, gy]), dev).to(tdt), T(np.concatenate([gy, x]), dev).to(tdt)
    ptr = torch.tensor([0, n, n, 2 * n], dtype=torch.int64, device=dev)

    def both(xs, gs, plan, ptr):
        xs, ts = xs.clone().requires_grad_(True), T(t, dev).to(rdt).requires_grad_(True)
        y, res = heat_diffuse(xs, ts, plan, ptr=ptr, iters=16, return_residual=True)
        return (y.detach(), res) + torch.autograd.grad(y, [xs, ts], gs)
    y, res, gx, gt = both(x2, g2, batch, ptr)
    assert res.shape == (3, 5) and not bool(res[1].any())
    gt_sum = 0
    for b, (lo, hi) in enumerate(((0, n), (n, 2 * n))):
        ya, ra, gxa, gta = both(x2[lo:hi].contiguous(), g2[lo:hi].contiguous(), single, None)
        assert same_bits(y[lo:hi], ya) and same_bits(gx[lo:hi], gxa) and same_bits(res[2 * b:2 * b + 1], ra)
        gt_sum = gt_sum + gta.double()
    assert float((gt.double() - gt_sum).abs().max()) <= 1e-6 * float(gt_sum.abs().max())          # (summed over the meshes in double)


def test_ring_beyond_the_lds_capacity(dev):
    """LDS_ROWS + 1 samples on a ring, two neighbours each: the search direction lives in the workspace"""
    from fieldconv_amd.diffusion import LDS_ROWS
    from fieldconv_amd.functional import diffusion_plan, heat_diffuse
    n = LDS_ROWS[torch.complex64] + 1
    rng = np.random.RandomState(2)
    a = np.arange(n)
    u = np.exp(1j * rng.uniform(-np.pi, np.pi, n))
    rows = np.concatenate([np.stack([a, (a + 1) % n], 1), np.stack([(a + 1) % n, a], 1)]).astype(np.int64)
    xp = np.concatenate([u, np.conj(u)]).astype(np.complex64)
    mag = np.tile(rng.uniform(0.1, 0.2, n), 2).astype(np.float32)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    ref = dref.Plan(rows, xp, mag, n, w, h=0.02)
    plan = diffusion_plan(T(rows), T(xp), T(mag), n, T(w), 0.02)
    vals = N_(plan.coef), N_(plan.coef_real), N_(plan.diag), N_(plan.diag_real)
    x, t = dref.features(n, 3, True, 3), np.array([0.5, 0.0, 2.0], dtype=np.float32)
    y = heat_diffuse(T(x, dev), T(t, dev), plan, iters=16)
    assert same_bits(y, heat_diffuse(T(x, dev), T(t, dev), plan, iters=16))
    gate(N_(y), dref.heat_diffuse(ref, x, t, np.float64, 16, values=vals), dref.heat_diffuse(ref, x, t, np.float32, 16, values=vals),
         np.float32, f'ring of {n} rows through the workspace')


# ------------------------------------------------------------------ 4. t = 0, a negative t, guard bands
def test_bad_times_and_guard_bands(dev, monkeypatch):
    from test_gpu_canary import GuardedTorch
    import fieldconv_amd._launch as launch
    import fieldconv_amd.diffusion as diffusion
    g = GuardedTorch()
    for mod in (launch, diffusion):
        monkeypatch.setattr(mod, 'torch', g)
    plan = build_plan()
    x, gy, t = inputs(5, True)
    t = t.copy()
    t[0], t[2], t[4] = 0, -1e-3, np.inf
    xd, td = T(x, dev).requires_grad_(True), T(t, dev).requires_grad_(True)
    y, res = diffusion.heat_diffuse(xd, td, plan, iters=4, return_residual=True)
    gx, gt = torch.autograd.grad(y, [xd, td], T(gy, dev))
    lap = diffusion.connection_laplacian(xd, plan)
    assert g.check('heat_diffuse, its backward pass and connection_laplacian') > 8
    bad = torch.tensor([False, False, True, False, True], device=dev)
    assert bool(torch.isnan(torch.view_as_real(y.detach())).all(-1)[:, bad].all()) and bool(torch.isfinite(torch.view_as_real(y.detach()))[:, ~bad].all())
    assert bool(torch.isnan(res[:, bad]).all()) and bool(torch.isfinite(res[:, ~bad]).all()) and bool(torch.isfinite(lap.detach().abs()).all())
    assert bool(torch.isfinite(gx.abs())[:, ~bad].all())
    assert same_bits(y.detach()[:, :2].contiguous(), xd.detach()[:, :2].contiguous()) and not bool(res[:, :2].any())
    # the good columns are the columns of a run without the bad ones
    keep = [0, 1, 3]
    y2 = diffusion.heat_diffuse(xd.detach()[:, keep].contiguous(), td.detach()[keep].contiguous(), plan, iters=4)
    assert same_bits(y.detach()[:, keep].contiguous(), y2)


# ------------------------------------------------------------------ 5. end to end: a lattice through the transforms, a StepGraph
EPSILON = 0.3


@functools.lru_cache(maxsize=None)
def lattice_data():
    from fieldconv_amd.transforms import ComputeLogXPort, DiffusionOperator, GeodesicSupportGraph
    pos, face = gref.lattice(9, 9)
    return DiffusionOperator()(ComputeLogXPort(EPSILON)(GeodesicSupportGraph(EPSILON)(SimpleNamespace(pos=T(pos), face=T(face)))))


def test_lattice_through_the_transforms_and_the_module(dev):
    from fieldconv_amd.nn import TangentDiffusion
    from fieldconv_amd.utils import StepGraph
    data = lattice_data()
    plan = data.diffusion_plan
    assert plan.n == 81 and plan.w is not None
    ref = dref.Plan(N_(data.supp_edges), N_(data.xp), N_(data.logMag), 81, N_(data.w).reshape(-1))
    assert plan.h == ref.h and np.array_equal(N_(plan.col), ref.col) and np.array_equal(N_(plan.edge), ref.edge)
    vals = N_(plan.coef), N_(plan.coef_real), N_(plan.diag), N_(plan.diag_real)
    scale = float(np.median(N_(plan.w)) / max(np.median(vals[2][vals[2] > 0]), 1e-30))          # t * diag ~ w: diffusion that matters
    C = 6
    layer = TangentDiffusion(C, iters=16, init_time=[scale * k for k in (0.0, 0.25, 0.5, 1.0, 2.0, 4.0)]).to(dev)
    assert list(layer.state_dict()) == ['time'] and layer.time.dtype == torch.float32
    x, gy = dref.features(81, C, True, 1), dref.features(81, C, True, 2)
    xd, gd = T(x, dev).requires_grad_(True), T(gy, dev)
    y = layer(xd, plan)
    gx, gt = torch.autograd.grad(y, [xd, layer.time], gd)
    y = y.detach()          # (no autograd graph of an eager run may be alive at capture time: utils/step_graph.py)
    t = N_(layer.time)
    for real in (np.float32,):
        want, own = dref.heat_diffuse(ref, x, t, np.float64, 16, values=vals), dref.heat_diffuse(ref, x, t, np.float32, 16, values=vals)
        gate(N_(y), want, own, real, 'lattice y')
        (wgx, wgt), (ogx, ogt) = (dref.heat_diffuse_backward(ref, x, t, gy, r, 16, values=vals) for r in (np.float64, np.float32))
        gate(N_(gx), wgx, ogx, real, 'lattice gx')
        gate(N_(gt), wgt, ogt, real, 'lattice gt')
    assert same_bits(y[:, 0].contiguous(), xd.detach()[:, 0].contiguous())
    yr = layer(T(x.real.copy(), dev), plan).detach()                             # real features through the same module
    gate(N_(yr), dref.heat_diffuse(ref, x.real.copy(), t, np.float64, 16, values=vals),
         dref.heat_diffuse(ref, x.real.copy(), t, np.float32, 16, values=vals), np.float32, 'lattice y, real features')

    def step():
        out = layer(xd, plan)
        return (out.detach(),) + torch.autograd.grad(out, [xd, layer.time], gd)
    graphed = StepGraph(step)
    for factor in (1.0, 0.5):
        with torch.no_grad():
            layer.time.mul_(factor)
        eager = [v.clone() for v in step()]
        assert all(same_bits(a, b) for a, b in zip(graphed.replay(), eager))          # the replay sees the new times
    assert not same_bits(eager[0], y)


def test_argument_errors_raise_before_any_launch(dev):
    from fieldconv_amd.functional import connection_laplacian, diffusion_plan, heat_diffuse
    plan = device_plan()
    x, _, t = inputs(5, True)
    xd, td = T(x, dev), T(t, dev)
    with pytest.raises(RuntimeError):
        heat_diffuse(xd.cpu(), td.cpu(), plan)
    with pytest.raises(RuntimeError):
        heat_diffuse(xd, td.cpu(), plan)
    with pytest.raises(TypeError):
        heat_diffuse(xd.real.to(torch.int32), td, plan)
    with pytest.raises(TypeError):
        connection_laplacian(xd.real.to(torch.float16), plan)
    with pytest.raises(ValueError):
        heat_diffuse(xd, td.double(), plan)
    with pytest.raises(ValueError):
        heat_diffuse(xd, td[:4], plan)
    for iters in (0, 1025, 2.5, True):
        with pytest.raises(ValueError):
            heat_diffuse(xd, td, plan, iters=iters)
    with pytest.raises(ValueError):
        heat_diffuse(xd, td, plan, ptr=torch.tensor([0, 30, 66], dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        heat_diffuse(xd[:66], td, plan)
    with pytest.raises(ValueError):
        heat_diffuse(xd, td, object())
    rows, xp, mag, w, n = dref.planted()
    with pytest.raises(ValueError):
        diffusion_plan(T(rows), T(xp), T(mag), n, T(w), h=-1.0)
    with pytest.raises(ValueError):
        diffusion_plan(T(rows), T(xp).to(torch.complex128), T(mag), n)
    with pytest.raises(ValueError):
        diffusion_plan(T(rows), T(xp), T(mag), 10)
