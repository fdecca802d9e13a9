"""TangentNorm on the device (fieldconv_amd.norm, csrc/fc_norm.hip, nn.TangentNorm) against the numpy restatement tests/_norm_ref.py.

The shapes are the smallest that reach every branch of the reduction: ptr = [0, 0, 1, 64, 129, 386] -- an empty mesh, a single
row, one row short of a chunk, one over, and five chunks, so that the finishing loop's stride of 4 wraps -- and C = 1, 48, 65:
below, inside and across the 64-channel tile.

complex64 values are gated as tests/test_gpu_transfer.py gates its own: against the float64 restatement, within 4 x the float32
restatement's own error, with a floor of 1e-6 of the largest entry; complex128 within 1e-12 of the largest entry."""
import functools

import numpy as np
import pytest
import torch

import _norm_ref as nref

pytestmark = pytest.mark.gpu

PTR = list(nref.STANDARD_PTR)
N = PTR[-1]
EPS = 1e-5
DTYPES = {'complex64': (torch.complex64, torch.float32, np.float32), 'complex128': (torch.complex128, torch.float64, np.float64)}


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


def within(name, got, want64, own32, real):
    """got against the float64 restatement: the project's gate for the 32-bit dtype, 1e-12 of the largest entry for the 64-bit one"""
    err = float(np.abs(got - want64).max())
    gate = gate_of(want64, own32) if real == np.float32 else 1e-12 * float(np.abs(want64).max())
    print(f'\n{name}: device against float64 {err:.3e}, gate {gate:.3e}')
    assert np.all(np.isfinite(got)) and err <= gate, (name, err, gate)


@functools.lru_cache(maxsize=None)
def inputs(C, weighted, gained):
    """(x, gy, w or None, gain or None): float32-representable, shared and never modified"""
    return (nref.features(N, C, 10 + C), nref.features(N, C, 20 + C), nref.weights(N, 30 + C) if weighted else None,
            nref.gains(C, 40 + C) if gained else None)


@functools.lru_cache(maxsize=None)
def reference(C, weighted, gained, real):
    """(y, gx, ggain) of the restatement in the arithmetic of `real`"""
    x, gy, w, gain = inputs(C, weighted, gained)
    return (nref.forward(x, PTR, w, gain, EPS, real),) + nref.backward(x, gy, PTR, w, gain, EPS, real)


def device_ptr(dev, ptr=PTR):
    from fieldconv_amd.pooling import tag_ptr
    return tag_ptr(torch.tensor(ptr, dtype=torch.int64).to(dev), ptr)          # as MeshBatch tags the tables it builds


def run(x, gy, w, gain, tdt, rdt, dev, ptr=PTR, eps=EPS):
    """(y, gx, ggain or None) of the device op"""
    from fieldconv_amd.norm import tangent_norm
    xd = T(x, dev).to(tdt).requires_grad_(True)
    gd = None if gain is None else T(gain, dev).to(rdt).reshape(1, -1).requires_grad_(True)
    wd = None if w is None else T(w, dev).to(rdt)
    y = tangent_norm(xd, gd, None if ptr is None else device_ptr(dev, ptr), wd, eps)
    grads = torch.autograd.grad(y, [xd] if gd is None else [xd, gd], T(gy, dev).to(tdt))
    return y.detach(), grads[0], (grads[1] if gd is not None else None)


# ------------------------------------------------------------------ 1. values, and the same bits twice
@pytest.mark.parametrize('gained', [False, True], ids=['no gain', 'gain'])
@pytest.mark.parametrize('weighted', [False, True], ids=['no w', 'w'])
@pytest.mark.parametrize('C', [1, 48, 65])
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_forward_and_gradients_equal_the_restatement(dev, dtype, C, weighted, gained):
    tdt, rdt, real = DTYPES[dtype]
    x, gy, w, gain = inputs(C, weighted, gained)
    y64, gx64, gg64 = reference(C, weighted, gained, np.float64)
    y32, gx32, gg32 = reference(C, weighted, gained, np.float32)
    y, gx, gg = run(x, gy, w, gain, tdt, rdt, dev)
    y2, gx2, gg2 = run(x, gy, w, gain, tdt, rdt, dev)
    assert y.dtype == tdt and tuple(y.shape) == (N, C) and gx.dtype == tdt and tuple(gx.shape) == (N, C)
    assert same_bits(y, y2) and same_bits(gx, gx2)                       # no atomics, a fixed order: forward and backward
    within(f'{dtype} C={C} forward', N_(y), y64, y32, real)
    within(f'{dtype} C={C} gx', N_(gx), gx64, gx32, real)
    if gained:
        assert gg.dtype == rdt and tuple(gg.shape) == (1, C) and same_bits(gg, gg2)
        within(f'{dtype} C={C} ggain', N_(gg)[0], gg64, gg32, real)


@pytest.mark.parametrize('weighted', [False, True], ids=['no w', 'w'])
def test_gradcheck(dev, weighted):
    from fieldconv_amd.norm import tangent_norm
    x = T(nref.features(7, 3, 8), dev).requires_grad_(True)
    gain = T(nref.gains(3, 9), dev).reshape(1, 3).requires_grad_(True)
    w = T(nref.weights(7, 10), dev) if weighted else None
    ptr = device_ptr(dev, [0, 3, 7])
    assert torch.autograd.gradcheck(lambda t, g: tangent_norm(t, g, ptr, w, 1e-3), (x, gain))


# ------------------------------------------------------------------ 2. a batch is its single meshes
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_batch_equals_the_single_meshes(dev, dtype):
    tdt, rdt, real = DTYPES[dtype]
    C = 65
    x, gy, w, gain = inputs(C, True, True)
    y, gx, gg = run(x, gy, w, gain, tdt, rdt, dev)
    total = np.zeros(C)
    for b in range(len(PTR) - 1):
        p0, p1 = PTR[b], PTR[b + 1]
        if p1 == p0:
            continue
        yb, gxb, ggb = run(x[p0:p1], gy[p0:p1], w[p0:p1], gain, tdt, rdt, dev, ptr=None)
        assert same_bits(y[p0:p1], yb) and same_bits(gx[p0:p1], gxb), f'mesh {b}'
        total += N_(ggb)[0].astype(np.float64)
    _, _, gg64 = reference(C, True, True, np.float64)
    _, _, gg32 = reference(C, True, True, np.float32)
    gate = gate_of(gg64, gg32) if real == np.float32 else 1e-12 * float(np.abs(gg64).max())
    assert np.abs(N_(gg)[0] - total).max() <= gate


# ------------------------------------------------------------------ 3. gauge and scale
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_a_change_of_frames_commutes_with_the_layer(dev, dtype):
    """multiplying row n by a unit phase u[n] multiplies y[n] by u[n]"""
    tdt, rdt, real = DTYPES[dtype]
    C = 48
    x, gy, w, gain = inputs(C, True, True)
    u = np.exp(1j * np.random.default_rng(3).uniform(-np.pi, np.pi, N))[:, None]
    turned = (x * u).astype(np.complex64).astype(np.complex128) if real == np.float32 else x * u          # what the device is given
    y, _, _ = run(turned, gy, w, gain, tdt, rdt, dev)
    want = u * reference(C, True, True, np.float64)[0]
    within(f'{dtype} gauge', N_(y), want, nref.forward(turned, PTR, w, gain, EPS, np.float32), real)


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_scale_invariance_and_unit_mean_square_without_eps(dev, dtype):
    tdt, rdt, real = DTYPES[dtype]
    C = 48
    x, gy, w, _ = inputs(C, True, False)
    want = nref.forward(x, PTR, w, None, 0.0, np.float64)
    scaled = (3.7 * x).astype(np.complex64).astype(np.complex128) if real == np.float32 else 3.7 * x
    own = nref.forward(scaled, PTR, w, None, 0.0, np.float32)
    y1, _, _ = run(x, gy, w, None, tdt, rdt, dev, eps=0.0)
    y2, _, _ = run(scaled, gy, w, None, tdt, rdt, dev, eps=0.0)
    within(f'{dtype} eps=0', N_(y1), want, nref.forward(x, PTR, w, None, 0.0, np.float32), real)
    within(f'{dtype} eps=0, 3.7 x', N_(y2), want, own, real)

    def mean_square(y):
        y = y.astype(np.complex128)
        return np.stack([(w[p0:p1, None] * np.abs(y[p0:p1]) ** 2).sum(0) / w[p0:p1].sum() for p0, p1 in zip(PTR, PTR[1:]) if p1 > p0])
    one = np.ones((4, C))
    within(f'{dtype} mean square', mean_square(N_(y1)), one, mean_square(nref.forward(x, PTR, w, None, 0.0, np.float32)), real)


# ------------------------------------------------------------------ 4. zero meshes
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_a_mesh_of_zero_features(dev, dtype):
    """y == 0 exactly; gx is finite and equals gain / sqrt(eps) * gy on the mesh"""
    tdt, rdt, real = DTYPES[dtype]
    C = 48
    x, gy, w, gain = inputs(C, True, True)
    x = x.copy()
    x[64:129] = 0
    y, gx, gg = run(x, gy, w, gain, tdt, rdt, dev)
    assert bool((torch.view_as_real(y[64:129]) == 0).all())
    want = (gain / np.sqrt(EPS))[None, :] * gy[64:129]
    own = nref.backward(x, gy, PTR, w, gain, EPS, np.float32)[0][64:129]
    within(f'{dtype} zero mesh gx', N_(gx)[64:129], want, own, real)
    assert bool(torch.isfinite(torch.view_as_real(gx)).all()) and bool(torch.isfinite(gg).all())
    within(f'{dtype} zero mesh, all gx', N_(gx), nref.backward(x, gy, PTR, w, gain, EPS, np.float64)[0],
           nref.backward(x, gy, PTR, w, gain, EPS, np.float32)[0], real)


@pytest.mark.parametrize('dtype', list(DTYPES))
def test_a_mesh_of_zero_weights(dev, dtype):
    """y = gain * x / sqrt(eps) on the mesh, and its gx has no second term"""
    tdt, rdt, real = DTYPES[dtype]
    C = 48
    x, gy, w, gain = inputs(C, True, True)
    w = w.copy()
    w[129:386] = 0
    y, gx, _ = run(x, gy, w, gain, tdt, rdt, dev)
    scale = (gain / np.sqrt(EPS))[None, :]
    within(f'{dtype} zero weights y', N_(y)[129:386], scale * x[129:386], nref.forward(x, PTR, w, gain, EPS, np.float32)[129:386], real)
    within(f'{dtype} zero weights gx', N_(gx)[129:386], scale * gy[129:386], nref.backward(x, gy, PTR, w, gain, EPS, np.float32)[0][129:386], real)
    within(f'{dtype} zero weights, all y', N_(y), nref.forward(x, PTR, w, gain, EPS, np.float64), nref.forward(x, PTR, w, gain, EPS, np.float32), real)


# ------------------------------------------------------------------ 5. the tensor contract
def test_only_inputs_that_require_a_gradient_get_one(dev):
    from fieldconv_amd.norm import tangent_norm
    x, gy, w, gain = inputs(48, True, True)
    ptr = device_ptr(dev)
    gyd = T(gy, dev).to(torch.complex64)
    full = run(x, gy, w, gain, torch.complex64, torch.float32, dev)
    for need_x, need_gain in ((True, False), (False, True), (False, False)):
        xd = T(x, dev).to(torch.complex64).requires_grad_(need_x)
        gd = T(gain, dev).to(torch.float32).reshape(1, -1).requires_grad_(need_gain)
        wd = T(w, dev).to(torch.float32).requires_grad_(need_x or need_gain)               # geometry: never a gradient
        y = tangent_norm(xd, gd, ptr, wd)
        assert same_bits(y.detach(), full[0])
        if not (need_x or need_gain):
            assert not y.requires_grad
            continue
        y.backward(gyd)
        assert wd.grad is None and (xd.grad is not None) == need_x and (gd.grad is not None) == need_gain
        if need_x:
            assert same_bits(xd.grad, full[1])
        if need_gain:
            assert same_bits(gd.grad, full[2])


def test_views_are_taken_by_value(dev):
    """a transposed x (and a transposed cotangent) gives the result of its contiguous copy, bit for bit"""
    from fieldconv_amd.norm import tangent_norm
    x, gy, w, gain = inputs(48, True, True)
    ptr, wd, gd = device_ptr(dev), T(w, dev).to(torch.float32), T(gain, dev).to(torch.float32)
    full = run(x, gy, w, gain, torch.complex64, torch.float32, dev)
    xt = T(x.T, dev).to(torch.complex64).t().requires_grad_(True)            # (N,C) view of a (C,N) tensor
    gyt = T(gy.T, dev).to(torch.complex64).t()
    assert not xt.is_contiguous() and not gyt.is_contiguous()
    y = tangent_norm(xt, gd, ptr, wd[:, None])                              # gain (C,), w (N,1)
    gx, = torch.autograd.grad(y, xt, gyt)
    assert same_bits(y.detach(), full[0]) and same_bits(gx, full[1])
    yc = tangent_norm(T(x, dev).to(torch.complex64).conj().resolve_conj().conj(), gd, ptr, wd)          # a lazy conjugate
    assert same_bits(yc, full[0])


def test_module_in_double_precision(dev):
    from fieldconv_amd.nn import TangentNorm
    x, gy, w, _ = inputs(48, True, False)
    m = TangentNorm(48).to(dev).double()
    y = m(T(x, dev), device_ptr(dev), T(w, dev))
    assert y.dtype == torch.complex128
    want = nref.forward(x, PTR, w, None, EPS, np.float64)
    assert np.abs(N_(y) - want).max() <= 1e-12 * np.abs(want).max()
    with pytest.raises(ValueError):                                          # a float32 gain beside complex128 features
        TangentNorm(48).to(dev)(T(x, dev))


# ------------------------------------------------------------------ 6. guard bands
@pytest.mark.parametrize('dtype', list(DTYPES))
def test_no_write_outside_any_buffer(dev, monkeypatch, dtype):
    """x, gy, w, gain, ptr, y, r, gx, ggain and both workspaces sit between guard bands (tests/test_gpu_canary.py); C = 65"""
    from test_gpu_canary import GuardedTorch
    import fieldconv_amd._launch as launch
    import fieldconv_amd.norm as norm
    from fieldconv_amd.pooling import tag_ptr
    tdt, rdt, real = DTYPES[dtype]
    g = GuardedTorch()
    monkeypatch.setattr(norm, 'torch', g)
    monkeypatch.setattr(launch, 'torch', g)

    def guarded_copy(t):
        out = g._guarded(tuple(t.shape), t.dtype, t.device)
        out.copy_(t)
        return out
    C = 65
    x, gy, w, gain = inputs(C, True, True)
    xd = guarded_copy(T(x, dev).to(tdt)).requires_grad_(True)
    gd = guarded_copy(T(gain, dev).to(rdt).reshape(1, -1)).requires_grad_(True)
    ptr = tag_ptr(guarded_copy(torch.tensor(PTR, dtype=torch.int64).to(dev)), PTR)
    y = norm.tangent_norm(xd, gd, ptr, guarded_copy(T(w, dev).to(rdt)))
    gx, gg = torch.autograd.grad(y, [xd, gd], guarded_copy(T(gy, dev).to(tdt)))
    assert g.check('tangent_norm') >= 11
    y64, gx64, gg64 = reference(C, True, True, np.float64)
    y32, gx32, gg32 = reference(C, True, True, np.float32)
    within(f'{dtype} guarded forward', N_(y), y64, y32, real)
    within(f'{dtype} guarded gx', N_(gx), gx64, gx32, real)
    within(f'{dtype} guarded ggain', N_(gg)[0], gg64, gg32, real)


# ------------------------------------------------------------------ 7. inside a captured step
def test_step_graph_replay_reproduces_the_eager_bits(dev):
    """TangentNorm on a tagged ptr (no synchronisation) and on ptr=None (the table built from the shape) inside one capture"""
    from fieldconv_amd.nn import TangentNorm
    from fieldconv_amd.utils import StepGraph
    x, gy, w, gain = inputs(48, True, True)
    m = TangentNorm(48).to(dev)
    with torch.no_grad():
        m.gain.copy_(T(gain, dev).to(torch.float32).reshape(1, -1))
    xd = T(x, dev).to(torch.complex64).requires_grad_(True)
    gyd, wd, ptr = T(gy, dev).to(torch.complex64), T(w, dev).to(torch.float32), device_ptr(dev)

    def step():
        y = m(xd, ptr, wd)
        z = m(xd)
        return (y.detach(), z.detach()) + torch.autograd.grad([y, z], [xd, m.gain], [gyd, gyd])
    eager = [t.clone() for t in step()]
    graphed = StepGraph(step)
    assert all(same_bits(a, b) for a, b in zip(eager, graphed.replay()))
    with torch.no_grad():                                                    # static addresses, fresh values
        xd.mul_(1.5)
    replayed = [t.clone() for t in graphed.replay()]
    assert all(same_bits(a, b) for a, b in zip(step(), replayed)) and not same_bits(replayed[2], eager[2])
