"""The TransField and ECHO descriptor kernels (csrc/fc_trans_field.hip, fc_echo.hip, fc_lift_echo_generic.hip), ROW BY ROW against the
oracle's torch restatement in float64 (inputs, references and masks: _lift_echo_cases.py, pinned on the CPU by
test_lift_echo_host.py).

Planted meshes put every in-degree at the edges of the prefetch groups, E // N on both sides of the wavefronts-per-vertex
thresholds and the last vertices into partly filled workgroups; the rows differ by powers of two, at random inside a workgroup and
workgroup by workgroup.  Every output -- y / desc and gx per vertex, the parameter gradients per output channel -- is measured by
rowwise_err and gated at 4 x the float32 restatement's own row-wise error (floor 1e-6; float64: 1e-12), computed per tensor and case.

Part two: rows do not leak into each other.  Rows that are neither perturbed nor fed by a perturbed row are BIT-IDENTICAL whatever
the perturbed rows hold -- times 2^40 or NaN (values, not faults)."""
import numpy as np
import pytest
import torch

import _lift_echo_cases as lc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def D(a, dev, dtype=None):
    t = torch.from_numpy(np.array(a))            # (a writable copy: the generator's arrays are read-only)
    return (t if dtype is None else t.to(dtype)).to(dev)


def check(label, got, own, f64=False):
    """the device's errors `got` within the gates that the restatement's errors `own` give, key by key; prints all three"""
    parts, bad = [], []
    for key, err in got.items():
        gate = lc.gate_of(own[key], f64)
        parts.append('%s %.2e (own %.2e, gate %.2e)' % (key, err, own[key], gate))
        if not err <= gate:
            bad.append(key)
    print('\n%s: %s' % (label, '  '.join(parts)))
    assert not bad, (label, bad)


# ---------------------------------------------------------------------------------------------- TransField
def tf_stencil(p, form, dev, f64=False):
    """The stencil of problem p in one of the forms the kernels read: 'packed' (E,R,2), 'strided2' / 'strided3' = columns B:B+2 of a full
    (E,R,2B+1) stencil whose other columns hold NaN, 'factors' = FCPrecomp's factor table behind its LiftColumns stand-in."""
    from fieldconv_amd.graph import FactoredStencil, LiftColumns
    s01 = D(p['s01'], dev, torch.complex128 if f64 else None)
    if form == 'packed':
        return s01
    if form.startswith('strided'):
        B = int(form[-1])
        full = torch.full((s01.shape[0], s01.shape[1], 2 * B + 1), float('nan'), dtype=s01.dtype, device=dev)
        full[..., B:B + 2] = s01
        view = full[..., B:B + 2]
        assert not view.is_contiguous() and view.stride(1) == 2 * B + 1
        return view
    lift = FactoredStencil(D(p['factors'], dev), s01.shape[1], 5, None)[..., 2:4]
    assert isinstance(lift, LiftColumns) and lift._dense is None
    return lift


def tf_run(p, ftype, dev, form='packed', f64=False, x=None, gy=None):
    from fieldconv_amd import functional as Fn
    real = torch.float64 if f64 else torch.float32
    xd = D(p['x'] if x is None else x, dev, real).requires_grad_(True)
    par = [D(p[k], dev, real).requires_grad_(True) for k in ('zonalAng', 'zonalMag', 'phase')]
    sten = tf_stencil(p, form, dev, f64)
    O, Cin, R = p['zonalAng'].shape
    assert Fn.trans_field_specialised(xd, sten, par[0]) == lc.tf_specialised(Cin, R, O, f64)
    y = Fn.trans_field(xd, D(p['edges'], dev), sten, par[0], par[1], par[2], ftype)
    wrt = [xd] + par[:3 if ftype else 2]
    grads = torch.autograd.grad(y, wrt, grad_outputs=D(p['gy'] if gy is None else gy, dev, torch.complex128 if f64 else None))
    return dict(zip(lc.TF_OUTPUTS, [H(y)] + [H(g) for g in grads]))


@pytest.mark.parametrize('name', list(lc.TF_CASES))
def test_trans_field_rowwise(name, dev):
    m, Cin, R, O, ftype, layout, f64 = lc.tf_case(name)
    p, want = lc.tf_problem(name), lc.tf_reference(name)
    own = lc.tf_errors(lc.tf_reference(name, 'f32'), want)
    got = tf_run(p, ftype, dev, f64=f64)
    assert all(np.isfinite(v.view(np.float64 if f64 else np.float32)).all() for v in got.values())
    check('TransField %s %s' % (name, (lc.MESHES[m][0], p['edges'].shape[0], Cin, R, O, ftype)), lc.tf_errors(got, want), own, f64)
    if name in lc.TF_FORM_CASES:
        for form in ('strided2', 'strided3'):
            other = tf_run(p, ftype, dev, form)
            assert all(np.array_equal(other[k], got[k]) for k in got), (name, form)          # the same rows, read in place
        check('TransField %s, factor table' % name, lc.tf_errors(tf_run(p, ftype, dev, 'factors'), want), own)


def test_trans_field_module_takes_the_same_path(dev):
    """nn.TransField on a strided view gives what the functional call on the packed copy gives, bit for bit"""
    from fieldconv_amd.nn import TransField
    name = 'rows-w2-32'
    m, Cin, R, O, ftype, layout, f64 = lc.tf_case(name)
    p = lc.tf_problem(name)
    mod = TransField(Cin, O, n_rings=R, ftype=ftype).to(dev)
    with torch.no_grad():
        for k, t in (('zonalAng', mod.zonalAng), ('zonalMag', mod.zonalMag), ('phase', mod.phase)):
            t.copy_(D(p[k], dev))
    y = mod(D(p['x'], dev), D(p['edges'], dev), tf_stencil(p, 'strided2', dev))
    assert np.array_equal(H(y), tf_run(p, ftype, dev)['y'])


@pytest.mark.parametrize('name', list(lc.TF_CONTAINMENT))
def test_trans_field_rows_do_not_leak(name, dev):
    m, Cin, R, O, ftype, layout, f64 = lc.tf_case(name)
    p, N = lc.tf_problem(name), lc.MESHES[m][0]
    P = lc.perturbed_set(N)
    fwd, bwd = lc.affected_rows(p['edges'], N, P)
    clean = tf_run(p, ftype, dev)
    check('TransField %s' % name, lc.tf_errors(clean, lc.tf_reference(name)), lc.tf_errors(lc.tf_reference(name, 'f32'), lc.tf_reference(name)))
    print('  %s: %d perturbed vertices; unaffected rows: y %d gx %d of %d' % (name, P.size, (~fwd).sum(), (~bwd).sum(), N))
    for label, value in (('2^40', None), ('nan', np.nan)):
        xp = np.array(p['x'])
        xp[P] = xp[P] * np.float32(2.0 ** lc.PERTURB_EXP) if value is None else np.float32(value)
        got = tf_run(p, ftype, dev, x=xp)
        assert np.array_equal(got['y'][~fwd], clean['y'][~fwd]), ('y rows without an in-edge from P changed', label)
        gp = np.array(p['gy'])
        gp[P] = gp[P] * np.float32(2.0 ** lc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = tf_run(p, ftype, dev, gy=gp)
        assert np.array_equal(got['gx'][~bwd], clean['gx'][~bwd]), ('gx rows without an out-edge into P changed', label)
        assert np.array_equal(got['y'], clean['y'])


# ---------------------------------------------------------------------------------------------- ECHO
def require_default_wpv():
    """The cases are planted for the library's own wavefront rule: skip, with the reason, when FC_ECHO_WPV overrides it."""
    from fieldconv_amd import _env
    forced = _env.active().get('FC_ECHO_WPV')
    if forced and int(forced):
        pytest.skip('FC_ECHO_WPV=%s overrides echo_waves_per_vertex: the planted row lengths are for the default rule' % forced)


def echo_run(p, n_bins, C, dev, c128=False, x=None, gd=None):
    from fieldconv_amd.nn import ECHO
    cplx = torch.complex128 if c128 else torch.complex64
    xd = D(p['x'] if x is None else x, dev, cplx).requires_grad_(True)
    desc = ECHO(C, n_bins).to(dev)(xd, D(p['edges'], dev), D(p['ln'], dev, cplx), D(p['wxp'], dev, cplx))
    gx, = torch.autograd.grad(desc, [xd], grad_outputs=D(p['gd'] if gd is None else gd, dev, torch.float64 if c128 else None))
    return dict(desc=H(desc), gx=H(gx))


def echo_check(name, got, f64):
    want = lc.echo_reference(name)
    own = dict(zip(('desc', 'gx'), lc.echo_errors(name, lc.echo_reference(name, 'f32'), want)))
    m, C, n_bins = lc.echo_case(name)[:3]
    _, okg, share = lc.echo_masks(name)
    check('ECHO %s %s left out: desc %.4f gx %.3f' % (name, (lc.MESHES[m][0], lc.echo_problem(name)['edges'].shape[0], C, n_bins), share, 1 - okg.mean()),
          dict(zip(('desc', 'gx'), lc.echo_errors(name, got, want))), own, f64)


@pytest.mark.parametrize('name', list(lc.ECHO_CASES))
def test_echo_rowwise(name, dev):
    from fieldconv_amd import _lib
    require_default_wpv()
    m, C, n_bins, layout, c128 = lc.echo_case(name)
    if n_bins <= 8:
        assert _lib.load().fc_echo_channel_block(n_bins) == lc.channel_block(n_bins)
    got = echo_run(lc.echo_problem(name), n_bins, C, dev, c128)
    assert all(np.isfinite(v.view(np.float64 if c128 else np.float32)).all() for v in got.values())
    echo_check(name, got, c128)


@pytest.mark.parametrize('name', list(lc.ECHO_CONTAINMENT))
def test_echo_rows_do_not_leak(name, dev):
    require_default_wpv()
    m, C, n_bins, layout, c128 = lc.echo_case(name)
    p, N = lc.echo_problem(name), lc.MESHES[m][0]
    P = lc.perturbed_set(N)
    fwd, bwd = lc.affected_rows(p['edges'], N, P)
    clean = echo_run(p, n_bins, C, dev)
    echo_check(name, clean, False)
    print('  %s: %d perturbed vertices; unaffected rows: desc %d gx %d of %d' % (name, P.size, (~fwd).sum(), (~bwd).sum(), N))
    for label, value in (('2^40', None), ('nan', np.nan)):
        xp = np.array(p['x'])
        xp[P] = xp[P] * np.float32(2.0 ** lc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = echo_run(p, n_bins, C, dev, x=xp)
        assert np.array_equal(got['desc'][~fwd], clean['desc'][~fwd]), ('desc rows without an in-edge from P changed', label)
        gp = np.array(p['gd'])
        gp[P] = gp[P] * np.float32(2.0 ** lc.PERTURB_EXP) if value is None else np.float32(value)
        got = echo_run(p, n_bins, C, dev, gd=gp)
        assert np.array_equal(got['gx'][~bwd], clean['gx'][~bwd]), ('gx rows without an out-edge into P changed', label)
        assert np.array_equal(got['desc'], clean['desc'])
