"""Max pooling by magnitude on the device (fieldconv_amd.transfer.tangent_transfer_max, fieldconv_amd.pooling.mesh_max,
nn.TangentMaxPool / nn.MeshMaxPool, csrc/fc_maxpool.hip) against the numpy restatement tests/_maxpool_ref.py.

The gates are those of tests/test_gpu_transfer.py.  Winners are integer decisions on keys that numpy restates bit for bit: exact.
Real-feature values are copies: bit for bit.  32-bit complex values and all 32-bit gradients: against the float64 restatement
evaluated on the same winners, within 4 x the float32 restatement's own error, with a floor of 1e-6 of the largest entry; the
64-bit dtypes within 1e-12 of the largest entry."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import _logmap_ref as lref
import _maxpool_ref as mref
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
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.is_floating_point():
        a, b = (t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32) for t in (a, b))
    return bool((a == b).all())


def gate_of(want64, own, real):
    top = float(np.abs(want64).max())
    if real == np.float64:
        return 1e-12 * top
    return max(4 * float(np.abs(own - want64).max()), 1e-6 * top)


def check_values(name, got, want64, own, real):
    err, gate = float(np.abs(got - want64).max()), gate_of(want64, own, real)
    print(f'\n{name}: device against float64 {err:.3e}, gate {gate:.3e}')
    assert err <= gate


# ------------------------------------------------------------------ 1. random plans
@functools.lru_cache(maxsize=None)
def plan_case(which):
    """(rows, phase, conj, n_out, n_in, empty rows)"""
    if which == 'pool':
        rows, _, phase, empty = tref.random_plan()
        return rows, phase, True, 40, 300, empty
    if which == 'unpool':
        rows, _, phase = tref.one_slot_plan()
        return rows, phase, False, 300, 40, []
    rng = np.random.default_rng(21)                            # 'long': one row of 3 000 slots over 500 inputs, one of 1 slot, one empty
    rows = np.stack((np.concatenate((np.zeros(3000, dtype=np.int64), [1])), rng.integers(0, 500, 3001)), 1).astype(np.int64)
    rows = rows[rng.permutation(3001)]
    return rows, np.exp(1j * rng.uniform(-np.pi, np.pi, 3001)).astype(np.complex64), False, 3, 500, [2]


@functools.lru_cache(maxsize=None)
def plan_inputs(which, complex_x, C):
    """(x with ties at the top, gy): float32-representable"""
    rows, _, _, n_out, n_in, _ = plan_case(which)
    dt = np.complex64 if complex_x else np.float32
    x = mref.plant_ties(rows, n_out, tref.features(n_in, C, complex_x, 10 + C).astype(dt), seed=C)
    return x, tref.features(n_out, C, complex_x, 20 + C).astype(dt)


@functools.lru_cache(maxsize=None)
def plan_reference(which, complex_x, C, real):
    """(arg, y64, y own, gx64, gx own): the winners by keys in `real`, the values on them in float64 and in `real`"""
    rows, phase, conj, n_out, n_in, _ = plan_case(which)
    x, gy = plan_inputs(which, complex_x, C)
    if not complex_x:
        x = x.astype(real)
    arg = mref.transfer_winners(rows, n_out, x, real)
    return (arg,) + tuple(f(r) for f in (lambda r: mref.transfer_forward(rows, phase, conj, x, arg, r),
                                         lambda r: mref.transfer_backward(rows, phase, conj, n_in, gy, arg, r)) for r in (np.float64, real))


def device_plan(which, dev):
    from fieldconv_amd.transfer import TransferPlan
    rows, phase, conj, n_out, n_in, _ = plan_case(which)
    weight = np.random.default_rng(5).standard_normal(len(rows)).astype(np.float32)          # never read by a max
    return TransferPlan(T(rows, dev), T(weight, dev), T(phase, dev), n_out=n_out, n_in=n_in, conj_phase=conj)


def run_plan(which, dtype, C, dev, plan=None):
    from fieldconv_amd.transfer import tangent_transfer_max
    tdt, real, complex_x = DTYPES[dtype]
    x, gy = plan_inputs(which, complex_x, C)
    plan = device_plan(which, dev) if plan is None else plan
    xd = T(x, dev).to(tdt).requires_grad_(True)
    y, rows_won = tangent_transfer_max(xd, plan, return_indices=True)
    gx, = torch.autograd.grad(y, xd, T(gy, dev).to(tdt))
    return y.detach(), rows_won, gx


def check_plan(which, dtype, C, dev):
    tdt, real, complex_x = DTYPES[dtype]
    rows, _, _, n_out, n_in, empty = plan_case(which)
    arg, y64, y_own, gx64, gx_own = plan_reference(which, complex_x, C, real)
    (y, won, gx), (y2, won2, gx2) = run_plan(which, dtype, C, dev), run_plan(which, dtype, C, dev)
    assert y.dtype == tdt and tuple(y.shape) == (n_out, C) and gx.dtype == tdt and tuple(gx.shape) == (n_in, C)
    assert won.dtype == torch.int64 and np.array_equal(N_(won), mref.winner_rows(rows, arg))          # exact, ties included
    assert same_bits(y, y2) and same_bits(gx, gx2) and torch.equal(won, won2)
    if empty:
        e = T(np.array(empty), dev)
        assert bool((torch.view_as_real(y[e]) == 0).all()) if complex_x else bool((y[e] == 0).all())
        assert bool((won[e] == -1).all())
    if complex_x:
        check_values(f'{which} {dtype} C={C} forward', N_(y), y64, y_own, real)
    else:
        assert same_bits(y, T(y_own, dev))                                                            # a copy: bit for bit
    check_values(f'{which} {dtype} C={C} gradient', N_(gx), gx64, gx_own, real)
    lost = np.ones((n_in, C), dtype=bool)
    lost[mref.winner_rows(rows, arg)[arg >= 0], np.nonzero(arg >= 0)[1]] = False
    g = N_(torch.view_as_real(gx) if complex_x else gx[..., None])
    assert np.all(g[lost] == 0)                                                                       # exactly zero where nothing was won


@pytest.mark.parametrize('C', [1, 5, 48, 64, 70])
@pytest.mark.parametrize('dtype', list(DTYPES))
@pytest.mark.parametrize('which', ['pool', 'unpool'])
def test_random_plan_forward_indices_and_gradient(dev, which, dtype, C):
    if which == 'pool':
        x = plan_inputs(which, DTYPES[dtype][2], C)[0]
        assert mref.top_ties(plan_case(which)[0], 40, x, DTYPES[dtype][1]) >= 3
    check_plan(which, dtype, C, dev)


# ------------------------------------------------------------------ 2. one long row
@pytest.mark.parametrize('dtype', ['complex64', 'float32', 'complex128'])
def test_one_row_of_three_thousand_slots(dev, dtype):
    rows = plan_case('long')[0]
    assert np.bincount(rows[:, 0], minlength=3).tolist() == [3000, 1, 0] and len(np.unique(rows[rows[:, 0] == 0, 1])) < 3000
    check_plan('long', dtype, 5, dev)


# ------------------------------------------------------------------ 3. a change of frames
@pytest.mark.parametrize('which', ['pool', 'unpool'])
def test_a_change_of_frames_keeps_the_winners(dev, which):
    """input row i times a unit p_i, the phases of its slots times conj(p_i) (p_i under conj_phase): the same winners, the same y.
    The keys of the members of a row differ by 2.5e-3 relative or more, far above what rotating an entry moves its key by."""
    from fieldconv_amd.transfer import TransferPlan, tangent_transfer_max
    rows, phase, conj, n_out, n_in, _ = plan_case(which)
    rng = np.random.default_rng(31)
    C = 6
    mag = 1 + 0.01 * np.stack([rng.permutation(n_in) for _ in range(C)], 1)
    x = (mag * np.exp(1j * rng.uniform(-np.pi, np.pi, (n_in, C)))).astype(np.complex64)
    p = np.exp(1j * rng.uniform(-np.pi, np.pi, n_in))
    turned = phase.astype(np.complex128) * (p[rows[:, 1]] if conj else np.conj(p[rows[:, 1]]))
    arg = mref.transfer_winners(rows, n_out, x, np.float32)
    y64 = mref.transfer_forward(rows, phase, conj, x, arg, np.float64)
    own = mref.transfer_forward(rows, phase, conj, x, arg, np.float32)
    weight = T(np.ones(len(rows), dtype=np.float32), dev)
    a = tangent_transfer_max(T(x, dev), TransferPlan(T(rows, dev), weight, T(phase, dev), n_out=n_out, n_in=n_in, conj_phase=conj), True)
    b = tangent_transfer_max(T((x * p[:, None]).astype(np.complex64), dev),
                             TransferPlan(T(rows, dev), weight, T(turned.astype(np.complex64), dev), n_out=n_out, n_in=n_in, conj_phase=conj), True)
    assert np.array_equal(N_(a[1]), mref.winner_rows(rows, arg)) and torch.equal(a[1], b[1])
    check_values(f'{which} original frames', N_(a[0]), y64, own, np.float32)
    check_values(f'{which} turned frames', N_(b[0]), y64, own, np.float32)          # the same y: the same yardstick, the same gate
    between = float(np.abs(N_(b[0]) - N_(a[0])).max())
    print(f'\n{which} turned against original frames: {between:.3e}, gate {gate_of(y64, own, np.float32):.3e}')
    assert between <= gate_of(y64, own, np.float32)


# ------------------------------------------------------------------ 4. a level of the sphere
@functools.lru_cache(maxsize=None)
def level(batched):
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    meshes = [lref.icosphere(3), lref.icosphere(2)]

    def chain(data):
        data = GeodesicSupportGraph(0.7, sample_n=128, random_start=False)(data)
        data = ComputeLogXPort(0.7)(data)
        return data, CoarsenSamples(32, 1.2)(data)
    if batched:
        return chain(MeshBatch.from_list([SimpleNamespace(pos=torch.from_numpy(p), face=torch.from_numpy(f)) for p, f in meshes]).to('cuda:0'))
    return [chain(SimpleNamespace(pos=T(p), face=T(f))) for p, f in meshes]


def test_level_max_pool_takes_the_largest_member_of_every_cell(dev):
    from fieldconv_amd.nn import TangentMaxPool, TangentUnpool
    fine, coarse = level(False)[0]
    assert fine.sample_idx.shape == (128,) and coarse.coarse.shape == (32,) and coarse.n_outside == 0
    x = T(tref.features(128, 6, True, 41).astype(np.complex64), dev)
    y = TangentMaxPool()(x, coarse)
    assert tuple(y.shape) == (32, 6)
    cell, mag = N_(coarse.cell), np.abs(N_(x).astype(np.complex128))
    want = np.stack([mag[cell == c].max(0) for c in range(32)])
    # |u| = 1 within the rounding of the phase (1e-6, tests/test_gpu_transfer.py) and one complex product
    assert np.abs(np.abs(N_(y).astype(np.complex128)) - want).max() <= 2e-6 * want.max()
    # unpool, then max pool: the identity.  Every member of a cell holds its coarse sample's value up to a phase, so the winners
    # are decided by the last bits of the device's unpooled features: they are restated from those, exactly.  On these winners
    # the chain is restated on the level's own plans (their rows, weights and complex64 phases) in float64 and in float32.
    from fieldconv_amd.transfer import tangent_transfer_max
    z = tref.features(32, 6, True, 42).astype(np.complex64)
    up = TangentUnpool()(T(z, dev), coarse)
    back, won = tangent_transfer_max(up, coarse.pool, return_indices=True)
    assert same_bits(back, TangentMaxPool()(up, coarse))
    (u_rows, u_w, u_ph), (p_rows, _, p_ph) = ((N_(t) for t in plan.rows()) for plan in (coarse.unpool, coarse.pool))
    arg = mref.transfer_winners(p_rows, 32, N_(up), np.float32)
    assert np.array_equal(N_(won), mref.winner_rows(p_rows, arg)) and np.array_equal(N_(coarse.cell)[N_(won)], np.arange(32)[:, None].repeat(6, 1))
    back64, back_own = (mref.transfer_forward(p_rows, p_ph, True, tref.transfer(u_rows, u_w, u_ph, False, 128, z, r), arg, r)
                        for r in (np.float64, np.float32))
    check_values('unpool then max pool against its restatement', N_(back), back64, back_own, np.float32)
    check_values('unpool then max pool against z', N_(back), z.astype(np.complex128), back_own, np.float32)
    for real_x in (T(tref.features(128, 6, False, 43).astype(np.float32), dev),):
        got = TangentMaxPool()(real_x, coarse)
        assert same_bits(got, torch.stack([real_x[coarse.cell == c].max(0).values for c in range(32)]))


def test_batch_equals_the_single_meshes(dev):
    from fieldconv_amd.nn import TangentMaxPool
    singles, (fine, coarse) = level(False), level(True)
    assert coarse.ptr.tolist() == [0, 32, 64] and fine.ptr.tolist() == [0, 128, 256]
    parts = [T(tref.features(128, 6, True, 44 + b).astype(np.complex64), dev).requires_grad_(True) for b in range(2)]
    gys = [T(tref.features(32, 6, True, 46 + b).astype(np.complex64), dev) for b in range(2)]
    alone = [TangentMaxPool()(p, c) for p, (_, c) in zip(parts, singles)]
    alone_g = [torch.autograd.grad(y, p, g)[0] for y, p, g in zip(alone, parts, gys)]
    x = torch.cat([p.detach() for p in parts]).requires_grad_(True)
    y = TangentMaxPool()(x, coarse)
    gx, = torch.autograd.grad(y, x, torch.cat(gys))
    assert same_bits(y.detach(), torch.cat([a.detach() for a in alone])) and same_bits(gx, torch.cat(alone_g))


# ------------------------------------------------------------------ 5. mesh_max
@functools.lru_cache(maxsize=None)
def mesh_reference(complex_x, C, real):
    """(x, ptr, g, idx, out64, out own, gx64, gx own)"""
    x, ptr = mref.mesh_case(C, complex_x, seed=C)
    if not complex_x:
        x = x.astype(real)
    g = tref.features(len(ptr) - 1, C, False, 50 + C).astype(np.float32)
    idx = mref.mesh_winners(x, ptr, real)
    return (x, ptr, g, idx) + tuple(f(r) for f in (lambda r: mref.mesh_forward(x, idx, r), lambda r: mref.mesh_backward(x, idx, g, r))
                                    for r in (np.float64, real))


def run_mesh(x, ptr, g, tdt, dev):
    from fieldconv_amd.pooling import mesh_max
    xd = T(x, dev).to(tdt).requires_grad_(True)
    out, idx = mesh_max(xd, torch.from_numpy(ptr), soft_abs=tdt.is_complex, return_indices=True)
    gx, = torch.autograd.grad(out, xd, T(g, dev).to(out.dtype))
    return out.detach(), idx, gx


@pytest.mark.parametrize('C', [1, 5, 64, 100])
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_mesh_max_values_indices_and_gradient(dev, dtype, C):
    tdt, real, complex_x = DTYPES[dtype]
    x, ptr, g, idx, out64, out_own, gx64, gx_own = mesh_reference(complex_x, C, real)
    assert (np.diff(ptr) == mref.MESH_ROWS).all()
    (out, got_idx, gx), second = run_mesh(x, ptr, g, tdt, dev), run_mesh(x, ptr, g, tdt, dev)
    assert out.dtype == (torch.float32 if real == np.float32 else torch.float64) and tuple(out.shape) == (7, C) and gx.dtype == tdt
    assert got_idx.dtype == torch.int64 and np.array_equal(N_(got_idx), idx)                          # exact, ties included
    assert all(same_bits(a, b) for a, b in zip((out, got_idx, gx), second))
    assert bool((out[0] == 0).all()) and bool((got_idx[0] == -1).all())                              # the empty mesh
    if complex_x:
        check_values(f'mesh_max {dtype} C={C} forward', N_(out), out64, out_own, real)
        assert bool((out[2] == 0).all())                                                              # its winner lies inside the origin box
    else:
        assert same_bits(out, T(out_own, dev))
    check_values(f'mesh_max {dtype} C={C} gradient', N_(gx), gx64, gx_own, real)
    flat = N_(torch.view_as_real(gx) if complex_x else gx[..., None])
    lost = np.ones(x.shape, dtype=bool)
    lost[idx[idx >= 0], np.nonzero(idx >= 0)[1]] = False
    assert np.all(flat[lost] == 0)
    for b in (4, 6):                                                                                  # a mesh alone: the same bits
        p0, p1 = int(ptr[b]), int(ptr[b + 1])
        o1, i1, g1 = run_mesh(x[p0:p1], np.array([0, p1 - p0]), g[b:b + 1], tdt, dev)
        assert same_bits(o1, out[b:b + 1]) and torch.equal(i1 + p0, got_idx[b:b + 1]) and same_bits(g1, gx[p0:p1])


def test_mesh_max_pool_module_and_a_device_ptr(dev):
    from fieldconv_amd.nn import MeshMaxPool
    from fieldconv_amd.pooling import mesh_max
    x, ptr = mref.mesh_case(5, True, seed=5)
    xd = T(x, dev)
    a = MeshMaxPool()(xd, T(ptr, dev))
    assert same_bits(a, mesh_max(xd, torch.from_numpy(ptr))) and not a.requires_grad
    r = T(x.real.copy(), dev)
    assert same_bits(MeshMaxPool(soft_abs=False)(r, T(ptr, dev))[1:], torch.stack([r[ptr[b]:ptr[b + 1]].max(0).values for b in range(1, 7)]))


# ------------------------------------------------------------------ 6. views and frozen inputs
def test_views_and_frozen_inputs(dev):
    """a non-contiguous x and a conjugate view are taken by value; an x that requires no gradient builds no graph"""
    from fieldconv_amd.pooling import mesh_max
    from fieldconv_amd.transfer import tangent_transfer_max
    plan = device_plan('pool', dev)
    x = T(plan_inputs('pool', True, 5)[0], dev)
    y, won = tangent_transfer_max(x, plan, return_indices=True)
    assert not y.requires_grad and not won.requires_grad
    assert same_bits(tangent_transfer_max(x.t().contiguous().t(), plan), y)
    assert same_bits(tangent_transfer_max(x.conj().resolve_conj().conj(), plan), y)
    assert same_bits(tangent_transfer_max(torch.cat((x, x), 1)[:, ::2][:, :5], plan)[:, :3], tangent_transfer_max(x[:, [0, 2, 4]].contiguous(), plan))
    with pytest.raises(RuntimeError):
        tangent_transfer_max(x.cpu(), plan)
    with pytest.raises(TypeError):
        tangent_transfer_max(x.real.to(torch.float16), plan)
    with pytest.raises(ValueError):
        tangent_transfer_max(x[:299], plan)
    ptr = torch.tensor([0, 100, 300])
    out = mesh_max(x, ptr)
    assert not out.requires_grad
    assert same_bits(mesh_max(x.t().contiguous().t(), ptr), out) and same_bits(mesh_max(x.conj().resolve_conj().conj(), ptr), out)
    with pytest.raises(ValueError):
        mesh_max(x, torch.tensor([0, 100, 299]))


# ------------------------------------------------------------------ 7. guard bands
def test_no_write_outside_any_buffer(dev, monkeypatch):
    """x, y, arg, gx, the partial buffers, out, index and every plan buffer sit between guard bands (tests/test_gpu_canary.py);
    ragged C, the 200-slot row, and rowptr / col entries out of range: clamped, or skipped, as documented"""
    from test_gpu_canary import GuardedTorch
    import fieldconv_amd._launch as launch
    import fieldconv_amd.pooling as pooling
    import fieldconv_amd.transfer as transfer
    g = GuardedTorch()
    for mod in (transfer, pooling, launch):
        monkeypatch.setattr(mod, 'torch', g)

    def guarded_copy(t):
        if t is None:
            return None
        out = g._guarded(tuple(t.shape), t.dtype, t.device)
        out.copy_(t)
        return out
    rows, phase, conj, n_out, n_in, _ = plan_case('pool')
    for dtype, C, foreign in (('complex64', 70, False), ('float32', 5, False), ('float32', 70, False), ('complex128', 5, False),
                              ('complex64', 5, True)):
        tdt, real, complex_x = DTYPES[dtype]
        plan = device_plan('pool', dev)
        for csr in (plan._fwd, plan._bwd):
            csr.rowptr, csr.col, csr.weight, csr.phase, csr.other = (guarded_copy(t) for t in (csr.rowptr, csr.col, csr.weight, csr.phase, csr.other))
        x, gy = plan_inputs('pool', complex_x, C)
        usable = np.ones(len(rows), dtype=bool)
        if foreign:          # the ends of rowptr past the slots (clamped: the same rows), some cols out of range (skipped)
            usable[[0, 17, 400, 899]] = False
            plan._fwd.rowptr[0], plan._fwd.rowptr[-1] = -7, len(rows) + 1000
            plan._fwd.col[T(np.nonzero(~usable)[0], dev)] = T(np.array([-1, n_in, 2 ** 31 - 1, -2 ** 31], dtype=np.int32), dev)
            plan._bwd.rowptr[0], plan._bwd.rowptr[-1] = -1, 2 ** 31 - 1
            plan._bwd.col[T(np.array([3, 500]), dev)] = T(np.array([-5, n_out], dtype=np.int32), dev)
        xd = guarded_copy(T(x, dev).to(tdt)).requires_grad_(True)
        y, won = transfer.tangent_transfer_max(xd, plan, return_indices=True)
        gx, = torch.autograd.grad(y, xd, guarded_copy(T(gy, dev).to(tdt)))
        assert g.check(f'tangent_transfer_max ({dtype}, C={C})') >= 14
        if foreign:
            r = rows[tref.grouped(rows)]
            k = mref.key(x, real)[r[:, 1]]
            k[~usable] = -1                                                                           # below every key: never a winner
            want = np.stack([r[np.where(r[:, 0] == o, k.T, -2).argmax(1), 1] if (r[:, 0] == o).any() else np.full(C, -1) for o in range(n_out)])
            assert np.array_equal(N_(won), want) and bool(torch.isfinite(torch.view_as_real(gx)).all())
        else:
            arg = plan_reference('pool', complex_x, C, real)[0]
            assert np.array_equal(N_(won), mref.winner_rows(rows, arg))
            check_values(f'guarded {dtype} C={C} gradient', N_(gx), *plan_reference('pool', complex_x, C, real)[3:], real)
    for dtype, C in (('complex64', 100), ('float32', 5), ('complex128', 5)):
        tdt, real, complex_x = DTYPES[dtype]
        x, ptr = mesh_reference(complex_x, C, real)[:2]
        xd = guarded_copy(T(x, dev).to(tdt)).requires_grad_(True)
        out, got = pooling.mesh_max(xd, guarded_copy(T(ptr, dev)), soft_abs=complex_x, return_indices=True)
        gx, = torch.autograd.grad(out, xd, guarded_copy(torch.ones_like(out)))
        assert g.check(f'mesh_max ({dtype}, C={C})') >= 8
        assert np.array_equal(N_(got), mref.mesh_winners(x, ptr, real))
