"""Tangent-feature pooling and unpooling on the device (fieldconv_amd.transfer, csrc/fc_transfer.hip, transforms.CoarsenSamples,
nn.TangentPool / nn.TangentUnpool) against the numpy restatement tests/_transfer_ref.py.

Values of the 32-bit dtypes are gated as tests/test_gpu_head.py and tests/test_gpu_logmap.py gate theirs: against the float64
restatement, within 4 x the float32 restatement's own error, with a floor of 1e-6 of the largest entry; the 64-bit dtypes within
1e-12 of the largest entry.  Cells and plan rows are integer decisions on fields that have the same bits everywhere: exact."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _logmap_ref as lref
import _transfer_ref as tref

pytestmark = pytest.mark.gpu

DTYPES = {'complex64': (torch.complex64, np.float32, True), 'float32': (torch.float32, np.float32, False),
          'complex128': (torch.complex128, np.float64, True), 'float64': (torch.float64, np.float64, False)}


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
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(torch.int64 if a.element_size() == 8 else torch.int32) ==
                                                               b.view(torch.int64 if b.element_size() == 8 else torch.int32)).all())


def gate_of(want64, own32):
    top = float(np.abs(want64).max())
    return max(4 * float(np.abs(own32 - want64).max()), 1e-6 * top)


# ------------------------------------------------------------------ 1. random plans
@functools.lru_cache(maxsize=None)
def plan_case(which):
    """(rows, weight, phase, conj, n_out, n_in, empty rows)"""
    if which == 'pool':
        rows, weight, phase, empty = tref.random_plan()
        return rows, weight, phase, True, 40, 300, empty
    rows, weight, phase = tref.one_slot_plan()
    return rows, weight, phase, False, 300, 40, []


@functools.lru_cache(maxsize=None)
def plan_reference(which, complex_x, C, real):
    """(x, gy, y, gx) of the restatement in the arithmetic of `real`; the inputs are float32-representable"""
    rows, weight, phase, conj, n_out, n_in, _ = plan_case(which)
    dt = np.complex64 if complex_x else np.float32
    x, gy = tref.features(n_in, C, complex_x, 10 + C).astype(dt), tref.features(n_out, C, complex_x, 20 + C).astype(dt)
    return x, gy, tref.transfer(rows, weight, phase, conj, n_out, x, real), tref.adjoint(rows, weight, phase, conj, n_in, gy, real)


def device_plan(which, dev):
    from fieldconv_amd.transfer import TransferPlan
    rows, weight, phase, conj, n_out, n_in, _ = plan_case(which)
    return TransferPlan(T(rows, dev), T(weight, dev), T(phase, dev), n_out=n_out, n_in=n_in, conj_phase=conj)


@pytest.mark.parametrize('C', [1, 5, 48, 64, 70])
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('which', ['pool', 'unpool'])
def test_random_plan_forward_and_gradient(dev, which, dtype, C):
    from fieldconv_amd.transfer import tangent_transfer
    tdt, real, complex_x = DTYPES[dtype]
    empty = plan_case(which)[6]
    x, gy, y64, gx64 = plan_reference(which, complex_x, C, np.float64)
    plan = device_plan(which, dev)

    def run():
        xd = T(x, dev).to(tdt).requires_grad_(True)
        y = tangent_transfer(xd, plan)
        gx, = torch.autograd.grad(y, xd, T(gy, dev).to(tdt))
        return y.detach(), gx
    (y, gx), (y2, gx2) = run(), run()
    assert y.dtype == tdt and tuple(y.shape) == y64.shape and gx.dtype == tdt and tuple(gx.shape) == x.shape
    assert same_bits(y, y2) and same_bits(gx, gx2)                       # no atomics, a fixed order: forward and backward
    if empty:
        assert bool((torch.view_as_real(y[T(np.array(empty), dev)]) == 0).all()) if complex_x else bool((y[T(np.array(empty), dev)] == 0).all())
    for name, got, want in (('forward', N_(y), y64), ('gradient', N_(gx), gx64)):
        err = float(np.abs(got - want).max())
        if real == np.float32:
            own = plan_reference(which, complex_x, C, np.float32)[2 if name == 'forward' else 3]
            gate = gate_of(want, own)
        else:
            gate = 1e-12 * float(np.abs(want).max())
        print(f'\n{which} {dtype} C={C} {name}: device against float64 {err:.3e}, gate {gate:.3e}')
        assert err <= gate


def test_views_and_frozen_inputs(dev):
    """a non-contiguous x and a conjugate view are taken by value; an x that requires no gradient builds no graph"""
    from fieldconv_amd.transfer import tangent_transfer
    plan = device_plan('pool', dev)
    x = T(tref.features(300, 6, True, 2).astype(np.complex64), dev)
    y = tangent_transfer(x, plan)
    assert not y.requires_grad
    assert same_bits(tangent_transfer(x.t().contiguous().t(), plan), y)
    assert same_bits(tangent_transfer(x.conj().resolve_conj().conj(), plan), y)
    with pytest.raises(RuntimeError):
        tangent_transfer(x.cpu(), plan)
    with pytest.raises(TypeError):
        tangent_transfer(x.real.to(torch.float16), plan)
    with pytest.raises(ValueError):
        tangent_transfer(x[:299], plan)


# ------------------------------------------------------------------ 2. adjoint identity, gradcheck
def test_adjoint_identity(dev):
    from fieldconv_amd.transfer import tangent_transfer
    for which in ('pool', 'unpool'):
        plan = device_plan(which, dev)
        x = T(tref.features(plan.n_in, 7, True, 5), dev)
        gy = T(tref.features(plan.n_out, 7, True, 6), dev)
        lhs = float((gy.conj() * tangent_transfer(x, plan)).sum().real)
        rhs = float((tangent_transfer(gy, plan.adjoint()).conj() * x).sum().real)
        assert plan.adjoint().n_out == plan.n_in and plan.adjoint()._fwd is plan._bwd          # shared buffers
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), float(gy.abs().sum()))


@pytest.mark.parametrize('dtype', [torch.float64, torch.complex128])
def test_gradcheck(dev, dtype):
    from fieldconv_amd.transfer import TransferPlan, tangent_transfer
    rng = np.random.default_rng(7)
    rows = np.stack((rng.integers(0, 12, 30), rng.integers(0, 7, 30)), 1).astype(np.int64)
    plan = TransferPlan(T(rows, dev), T(rng.standard_normal(30), dev), T(np.exp(1j * rng.uniform(-3, 3, 30)), dev), n_out=12, n_in=7,
                        conj_phase=True)
    x = T(tref.features(7, 3, dtype.is_complex, 8), dev).to(dtype).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: tangent_transfer(t, plan), (x,))


# ------------------------------------------------------------------ 3. the sphere level pair
FINE_EPS, COARSE_EPS = 0.5, 0.95


@functools.lru_cache(maxsize=None)
def sphere(diagonals):
    """(fine data, coarse data, restated Level, pos, face): a 642-vertex icosphere, 256 geodesic-FPS fine samples, 64 coarse"""
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    pos, face = lref.icosphere(3)
    fine = SimpleNamespace(pos=T(pos), face=T(face))
    fine = GeodesicSupportGraph(FINE_EPS, sample_n=256, random_start=False, diagonals=diagonals)(fine)
    fine = ComputeLogXPort(FINE_EPS, diagonals=diagonals)(fine)
    coarse = CoarsenSamples(64, COARSE_EPS, diagonals=diagonals)(fine)
    level = tref.Level(pos, face, N_(fine.sample_idx), N_(coarse.coarse), N_(fine.w), diagonals)
    return fine, coarse, level, pos, face


def plan_rows(plan):
    rows, weight, phase = plan.rows()
    return N_(rows), N_(weight), N_(phase)


@pytest.mark.parametrize('diagonals', [False, True])
def test_sphere_cells_and_plans_equal_the_restatement(dev, diagonals):
    from fieldconv_amd.transfer import sample_cells
    fine, coarse, level, pos, face = sphere(diagonals)
    assert fine.sample_idx.shape == (256,) and coarse.coarse.shape == (64,) and bool((coarse.coarse[1:] > coarse.coarse[:-1]).all())
    assert torch.equal(coarse.sample_idx, fine.sample_idx[coarse.coarse])
    cell, dist = sample_cells(fine.pos, fine.face, fine.sample_idx, coarse.coarse, diagonals=diagonals)
    assert np.array_equal(N_(cell), level.cell) and np.array_equal(N_(dist).view(np.uint32), level.dist.view(np.uint32))
    assert torch.equal(coarse.cell, cell) and coarse.n_outside == 0 == level.n_outside
    assert np.array_equal(level.cell[N_(coarse.coarse)], np.arange(64))          # every coarse sample lies in its own cell
    for plan, rows in ((coarse.pool, level.pool_rows), (coarse.unpool, level.unpool_rows)):
        order = tref.grouped(rows)
        got_rows, got_w, got_ph = plan_rows(plan)
        assert np.array_equal(got_rows, rows[order])
        want_w = level.weight[order] if plan is coarse.pool else np.ones(len(rows), dtype=np.float32)
        # W_c is a fixed-order float32 sum with the restatement's bits; the one division may round the other way: 1 ulp
        assert np.allclose(got_w, want_w, rtol=2.0 ** -23, atol=0)
        x64 = level.xp(np.float64)[order]
        assert np.abs(got_ph - x64).max() <= max(4 * np.abs(level.xp(np.float32)[order] - x64).max(), 1e-6)
    assert coarse.pool.conj_phase and not coarse.unpool.conj_phase
    sums = np.bincount(level.c, weights=plan_rows(coarse.pool)[1][np.argsort(tref.grouped(level.pool_rows))].astype(np.float64), minlength=64)
    assert np.abs(sums - 1).max() <= 1e-6


@pytest.mark.parametrize('diagonals', [False, True])
def test_pool_of_unpool_is_the_identity(dev, diagonals):
    from fieldconv_amd.nn import TangentPool, TangentUnpool
    _, coarse, _, _, _ = sphere(diagonals)
    for complex_x in (True, False):
        y = T(tref.features(64, 5, complex_x, 11).astype(np.complex64 if complex_x else np.float32), dev)
        up = TangentUnpool()(y, coarse)
        assert tuple(up.shape) == (256, 5)
        back = TangentPool()(up, coarse)
        assert float((back - y).abs().max()) <= 1e-6 * float(y.abs().max())


# ------------------------------------------------------------------ 4. a flat grid: unit phases, the mass-weighted mean
def test_flat_grid_pools_the_mass_weighted_cell_mean(dev):
    from fieldconv_amd.geodesic import sample_weights
    from fieldconv_amd.transfer import level_transfer, tangent_transfer
    pos, face = tref.flat_grid(12)
    samples = np.arange(144, dtype=np.int64)
    coarse = np.array([13, 16, 19, 22, 49, 52, 55, 58, 85, 88, 91, 94, 121, 124, 127, 130], dtype=np.int64)
    p, f, s = T(pos, dev), T(face, dev), T(samples, dev)
    w = sample_weights(p, f, s)
    pool, unpool, cell, n_outside = level_transfer(p, f, s, T(coarse, dev), w, return_cells=True)
    assert n_outside == 0
    for plan in (pool, unpool):
        assert float((plan.rows()[2] - 1).abs().max()) <= 1e-6                       # all frames are equal
    x = tref.features(144, 5, True, 12).astype(np.complex64)
    got = N_(tangent_transfer(T(x, dev), pool))
    cell_n, w_n = N_(cell), N_(w).reshape(-1).astype(np.float64)
    want = np.zeros((16, 5), dtype=np.complex128)
    np.add.at(want, cell_n, w_n[:, None] * x)
    want /= np.bincount(cell_n, weights=w_n, minlength=16)[:, None]
    # every coefficient is off by at most 1e-6 (the phase) + 2 roundings, the weights sum to 1 and a cell of at most 16 members
    # adds 16 roundings: (1e-6 + 18 * 2^-24) of the largest entry, doubled
    assert np.abs(got - want).max() <= 4.2e-6 * np.abs(x).max()


# ------------------------------------------------------------------ 5. fine samples in no cell
def test_samples_outside_every_cell(dev):
    from fieldconv_amd.transfer import level_transfer, tangent_transfer
    pos, face, _ = gref.union([gref.lattice(5, 6), gref.lattice(4, 4)])
    p, f, s = T(pos, dev), T(face, dev), torch.arange(46, device=dev)
    coarse = torch.tensor([2, 17, 25], device=dev)
    pool, unpool, cell, n_outside = level_transfer(p, f, s, coarse, torch.ones(46, 1, device=dev), return_cells=True)
    cell = N_(cell)
    assert n_outside == 16 and np.all(cell[30:] == -1) and np.all(cell[:30] >= 0)
    assert np.array_equal(cell, tref.sample_cells(pos, face, np.arange(46), np.array([2, 17, 25]))[0])
    y = T(tref.features(3, 4, True, 13).astype(np.complex64), dev)
    up = tangent_transfer(y, unpool)
    assert bool((torch.view_as_real(up[30:]) == 0).all()) and bool((up[:30].abs() > 0).all())
    x = T(tref.features(46, 4, True, 14).astype(np.complex64), dev)
    other = x.clone()
    other[30:] = complex(float('nan'), float('nan'))                               # never read: they are in no row
    a, b = tangent_transfer(x, pool), tangent_transfer(other, pool)
    assert same_bits(a, b) and bool(torch.isfinite(torch.view_as_real(b)).all())


# ------------------------------------------------------------------ 6. a batch of two meshes
def test_batch_equals_the_single_meshes(dev):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    meshes = [lref.icosphere(3), lref.icosphere(2)]
    assert [m[0].shape[0] for m in meshes] == [642, 162]

    def chain(data):
        data = GeodesicSupportGraph(0.7, sample_n=96, random_start=False)(data)
        data = ComputeLogXPort(0.7)(data)
        return data, CoarsenSamples(20, 1.2)(data)
    singles = [chain(SimpleNamespace(pos=T(p, dev), face=T(f, dev))) for p, f in meshes]
    fine, coarse = chain(MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(p), face=torch.from_numpy(f)) for p, f in meshes]).to(dev))
    assert coarse.ptr.tolist() == [0, 20, 40] and fine.ptr.tolist() == [0, 96, 192] and coarse.num_meshes == 2
    f_off, c_off, v_off = [0, 96], [0, 20], [0, 642]
    cat = lambda parts: torch.cat(parts)
    shift = lambda t, o: torch.where(t >= 0, t + o, t)
    assert torch.equal(coarse.coarse, cat([c.coarse + o for (_, c), o in zip(singles, f_off)]))
    assert torch.equal(coarse.sample_idx, cat([c.sample_idx + o for (_, c), o in zip(singles, v_off)]))
    assert torch.equal(coarse.cell, cat([shift(c.cell, o) for (_, c), o in zip(singles, c_off)]))
    assert torch.equal(coarse.supp_edges, cat([c.supp_edges + o for (_, c), o in zip(singles, c_off)]))
    assert same_bits(coarse.w, cat([c.w for _, c in singles]))
    assert coarse.n_outside == 0
    for name, offs in (('pool', (c_off, f_off)), ('unpool', (f_off, c_off))):
        rows, weight, phase = getattr(coarse, name).rows()
        parts = [getattr(c, name).rows() for _, c in singles]
        want = cat([r + torch.tensor([offs[0][b], offs[1][b]], device=dev) for b, (r, _, _) in enumerate(parts)])
        assert torch.equal(rows, want)
        assert same_bits(weight, cat([w for _, w, _ in parts])) and same_bits(phase, cat([ph for _, _, ph in parts]))
    assert int(torch.div(coarse.pool.rows()[0][:, 1], 96, rounding_mode='floor').ne(torch.div(coarse.pool.rows()[0][:, 0], 20, rounding_mode='floor')).sum()) == 0


# ------------------------------------------------------------------ 7. end to end
def test_encoder_decoder_on_the_sphere_pair(dev):
    """FieldConv(8,8) on the fine level, pool, FieldConv(8,8) on the coarse level with its own FCPrecomp, unpool, added to the fine
    features; forward and backward.  The device's plans against the float64 restatement's plans cast to float32, gated as
    tests/test_gpu_logmap.py gates its end-to-end case: 4 x what the float32 restatement's plans give against the float64 ones,
    floor 1e-6 of the largest entry.
    Measured once on an MI355X: output 3.7e-9 (largest entry 9.6e-2), the six parameter gradients 8.9e-8, 1.5e-7, 3.0e-8, 3.7e-9,
    6.5e-9 and 8.1e-10 (largest entries 0.71, 1.03, 0.20, 2.5e-2, 3.6e-2, 4.5e-3) -- figure for figure what the float32 restatement's
    plans give: the device's phases are the float32 restatement's."""
    from fieldconv_amd.nn import FieldConv, TangentPool, TangentUnpool
    from fieldconv_amd.transfer import TransferPlan
    from fieldconv_amd.transforms import FCPrecomp
    fine, coarse, level, _, _ = sphere(False)
    torch.manual_seed(0)
    conv_f, conv_c = FieldConv(8, 8, band_limit=2, n_rings=6).to(dev), FieldConv(8, 8, band_limit=2, n_rings=6).to(dev)
    e_f, s_f = FCPrecomp(2, 6, FINE_EPS)(fine)[:2]
    e_c, s_c = FCPrecomp(2, 6, COARSE_EPS)(coarse)[:2]
    x = torch.randn(256, 8, dtype=torch.complex64).to(dev)
    go = torch.randn(256, 8, dtype=torch.complex64).to(dev)
    params = list(conv_f.parameters()) + list(conv_c.parameters())
    pool_op, unpool_op = TangentPool(), TangentUnpool()

    def run(lv):
        for p in params:
            p.grad = None
        h = conv_f(x, e_f, s_f)
        out = h + unpool_op(conv_c(pool_op(h, lv), e_c, s_c), lv)
        out.backward(go)
        return [N_(out)] + [N_(p.grad) for p in params if p.grad is not None]

    def restated(real):
        ph = T(level.xp(real).astype(np.complex64), dev)
        ones = T(np.ones(len(level.member), dtype=np.float32), dev)
        return SimpleNamespace(pool=TransferPlan(T(level.pool_rows, dev), T(level.weight, dev), ph, n_out=64, n_in=256, conj_phase=True),
                               unpool=TransferPlan(T(level.unpool_rows, dev), ones, ph, n_out=256, n_in=64))
    got, want, own = run(coarse), run(restated(np.float64)), run(restated(np.float32))
    assert len(got) >= 3
    for k, (g, w, o) in enumerate(zip(got, want, own)):
        top = float(np.abs(w).max())
        err, own_err = float(np.abs(g - w).max()), float(np.abs(o - w).max())
        gate = max(4 * own_err, 1e-6 * top)
        print(f'\n{"output" if k == 0 else f"gradient {k}"}: device plans {err:.3e}, float32 restatement plans {own_err:.3e}, gate {gate:.3e}, '
              f'largest entry {top:.3e}')
        assert err <= gate


# ------------------------------------------------------------------ 8. guard bands
def test_no_write_outside_any_buffer(dev, monkeypatch):
    """x, y, gx and every plan buffer sit between guard bands (tests/test_gpu_canary.py); C = 70 and the 200-slot row"""
    from test_gpu_canary import GuardedTorch
    import fieldconv_amd._launch as launch
    import fieldconv_amd.transfer as transfer
    g = GuardedTorch()
    monkeypatch.setattr(transfer, 'torch', g)
    monkeypatch.setattr(launch, 'torch', g)

    def guarded_copy(t):
        if t is None:
            return None
        out = g._guarded(tuple(t.shape), t.dtype, t.device)
        out.copy_(t)
        return out
    for which in ('pool', 'unpool'):
        plan = device_plan(which, dev)
        for csr in (plan._fwd, plan._bwd):
            csr.rowptr, csr.col, csr.weight, csr.phase = (guarded_copy(t) for t in (csr.rowptr, csr.col, csr.weight, csr.phase))
        x, gy, y64, gx64 = plan_reference(which, True, 70, np.float64)
        xd = guarded_copy(T(x, dev)).requires_grad_(True)
        y = transfer.tangent_transfer(xd, plan)
        gx, = torch.autograd.grad(y, xd, guarded_copy(T(gy, dev)))
        assert g.check(f'tangent_transfer ({which})') >= 8
        assert np.abs(N_(y) - y64).max() <= gate_of(y64, plan_reference(which, True, 70, np.float32)[2])
        assert np.abs(N_(gx) - gx64).max() <= gate_of(gx64, plan_reference(which, True, 70, np.float32)[3])
