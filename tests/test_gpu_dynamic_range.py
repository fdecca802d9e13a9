"""Per-row scaling of the record-driven kernels, ROW BY ROW (inputs and references: _dynamic_range_cases.py, pinned on the CPU
by test_dynamic_range_host.py).

The default arithmetic mode carries every contraction operand as two f16 halves with one power-of-two scale per row
(csrc/fc_tile.hpp, split_scale).  The scale is found, applied and divided out in the frequency-major forward kernels, in the
ring-major forward kernel (flush_row / contract), in the data / filter kernel pair (row scale, column scale colmag), in the
streaming gather (row scale of H, inverse scale 0 for zero rows), in the streaming kernel's second operand of gW (pair_max /
pair_rows) and in the filter images (fc_pack.hip, row_max2).  A global max-norm lets the large rows hide the small ones, so here
x and gy rows, filter rows and filter columns differ by powers of two -- at random inside a 16-vertex tile, and tile by tile --
under global exponents near both ends of the fp32 range, and every output is measured row by row against the complex128 oracle.

Part two: rows do not leak into each other.  y[n] depends on the x rows of n's in-neighbours only, gx[j] on x[j] and the gy rows
of j's out-neighbours only; summation orders are fixed and scales are per row, so such rows are BIT-IDENTICAL whatever happens
to the other rows -- times 2^40, inf or NaN (values, not faults)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _dynamic_range_cases as drc
from oracle import fieldconv_oracle as orc

pytestmark = pytest.mark.gpu
REDUCED = os.environ.get('FC_MFMA') == 'f16'
TOL = 5e-3 if REDUCED else 1e-5          # the gates of test_gpu_parity.py::test_dynamic_range_rowwise: y < TOL, gx < 5 TOL, gW < TOL


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def build_graph(name, dev):
    from fieldconv_amd.graph import SupportGraph
    edges, sten = drc.mesh(name)[:2]
    return SupportGraph(torch.from_numpy(edges).to(dev), torch.from_numpy(sten).to(dev), drc.SHAPES[name][0])


def require_kernels(name, graph, expect):
    """Assert from the library's own account that these dims take the kernels the case is meant for -- or skip, with the reason,
    when a mode run or a development switch has redirected them.  Returns the description."""
    from fieldconv_amd import _env, _lib
    from fieldconv_amd.functional import make_dims
    N, k, I, O, B, R = drc.SHAPES[name]
    lib = _lib.load()
    dims = make_dims(graph, I, O, B)
    kind = 2 if getattr(graph, 'geo_t', None) is not None else (1 if graph.factored else 0)
    buf = ctypes.create_string_buffer(1024)
    assert lib.fc_describe_kernels(ctypes.byref(dims), kind, buf, len(buf)) == 0
    desc = buf.value.decode()
    fwd, bwd = desc.split(';', 1)
    parts = re.search(r'parts=(\d+)', fwd)
    found = {
        'records': kind >= 1,
        'geometric': kind == 2,
        'generic': kind == 1,
        'frequency-major': 'frequency-major' in fwd,
        'edge-split': parts is not None and int(parts.group(1)) > 1,
        'ring-major': 'ring-major' in fwd,
        'kernel-pair': 'fc_backward_data_kernel<records' in bwd,
        'streaming': bool(lib.fc_backward_streams(ctypes.byref(dims), 1 if kind else 0)) and 'fc_backward_gather_kernel' in bwd,
    }
    missing = [e for e in expect if not found[e]]
    switches = {key: v for key, v in _env.active().items() if key != 'FIELDCONV_NO_GEO'}        # (that one is a case of this module)
    if missing and switches:
        pytest.skip('%s not selected under %s: %s' % (missing, switches, desc))
    assert not missing, (missing, desc)
    print('%s %s: %s' % (name, drc.SHAPES[name], desc))
    return desc


def run_explicit(graph, x, gy, W, dev):
    from fieldconv_amd.functional import field_conv
    xd = torch.from_numpy(x).to(dev).requires_grad_(True)
    Wd = torch.from_numpy(W).to(dev).requires_grad_(True)
    y = field_conv(xd, Wd, graph)
    gx, gW = torch.autograd.grad(y, [xd, Wd], grad_outputs=torch.from_numpy(gy).to(dev))
    return H(y), H(gx), H(gW)


def check(name, layout, gname, got, ref, tag=''):
    assert all(np.isfinite(t.view(np.float32)).all() for t in got), (name, layout, gname, tag)
    ey, egx, egw = drc.errors(name, layout, got, ref)
    print(f'  {name} {layout} x-gy {gname}{tag}: row-wise errors y {ey:.2e} gx {egx:.2e} gW {egw:.2e}')
    return ey, egx, egw


# kernels each shape is meant for
RECORD_CASES = [
    pytest.param('rec400', ('records', 'geometric', 'frequency-major', 'kernel-pair'), False, id='fm-pair-geometric-400'),
    pytest.param('rec400', ('records', 'generic', 'frequency-major', 'kernel-pair'), True, id='fm-pair-generic-400'),
    pytest.param('split60', ('records', 'frequency-major', 'edge-split', 'kernel-pair'), False, id='edge-split-60'),
    pytest.param('ring4400', ('records', 'ring-major', 'streaming'), False, id='ring-stream-default-4400'),
    pytest.param('ring4400pad', ('records', 'ring-major'), False, id='ring-padded-K-4400'),
    pytest.param('ring5000', ('records', 'ring-major'), False, id='ring-5000'),
    pytest.param('stream3100', ('records', 'streaming'), False, id='stream-smallest-3100'),
    pytest.param('stream3075', ('records', 'streaming'), False, id='stream-two-walks-3075'),
]


@pytest.mark.parametrize('xg', ['unit', 'tiny', 'huge'])
@pytest.mark.parametrize('layout', drc.LAYOUTS)
@pytest.mark.parametrize('name,expect,no_geo', RECORD_CASES)
def test_rowwise_accuracy_on_every_scaling_site(name, expect, no_geo, layout, xg, dev, monkeypatch):
    if no_geo:
        monkeypatch.setenv('FIELDCONV_NO_GEO', '1')
    graph = build_graph(name, dev)
    require_kernels(name, graph, expect)
    worst = [0.0, 0.0, 0.0]
    for gname, (gX, gG) in drc.GLOBALS.items():
        if not gname.startswith(xg):
            continue
        drc.assert_reference_in_range(name, layout, gX, gG, gname)            # (a condition on the inputs; the host test asserts it too)
        got = run_explicit(graph, *drc.scaled_inputs(name, layout, gX, gG), dev)
        errs = check(name, layout, gname, got, drc.scaled_reference(name, layout, gX, gG))
        worst = [max(w, e) for w, e in zip(worst, errs)]
    assert worst[0] < TOL and worst[1] < 5 * TOL and worst[2] < TOL, worst


def test_fp32_mode_control(dev):
    """The smallest record case once more in fp32 arithmetic, in the same process."""
    import fieldconv_amd
    name = 'split60'
    graph = build_graph(name, dev)
    with fieldconv_amd.arithmetic('f32'):
        desc = require_kernels(name, graph, ('records', 'frequency-major', 'kernel-pair'))       # (the dims carry the block's mode)
        assert 'f32' in desc.split(';', 1)[1], desc
        for layout in drc.LAYOUTS:
            for gname, (gX, gG) in drc.GLOBALS.items():
                got = run_explicit(graph, *drc.scaled_inputs(name, layout, gX, gG), dev)
                ey, egx, egw = check(name, layout, gname, got, drc.scaled_reference(name, layout, gX, gG), ' [f32]')
                assert ey < 1e-5 and egx < 5e-5 and egw < 1e-5


PARAM_KERNELS = {'param400': ('records', 'frequency-major', 'kernel-pair'), 'ring4400': ('records', 'ring-major', 'streaming')}


@pytest.mark.parametrize('name,ftype', drc.PARAM_CASES, ids=['%s-ftype%d' % c for c in drc.PARAM_CASES])
def test_parameter_path_filter_row_scales(name, ftype, dev):
    """zonal / spherical rows and columns scaled by the same powers of two; parameter gradients against the oracle's chain rule,
    row-wise over their leading axis."""
    from fieldconv_amd.nn import FieldConv
    N, k, I, O, B, R = drc.SHAPES[name]
    layout = 'random'
    graph = build_graph(name, dev)
    require_kernels(name, graph, PARAM_KERNELS[name])
    edges, sten = (torch.from_numpy(t).to(dev) for t in drc.mesh(name)[:2])
    z, s, p = drc.scaled_params(name, layout, ftype)
    conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=ftype)
    conv.load_state_dict({'zonal': torch.from_numpy(z), 'spherical': torch.from_numpy(s), 'phase': torch.from_numpy(p)})
    conv = conv.to(dev)
    names = [n for n, _ in conv.named_parameters()]
    assert names == ['zonal', 'spherical', 'phase'][:len(names)]
    worst = {}
    for gname in drc.PARAM_GLOBALS:
        gX, gG = drc.GLOBALS[gname]
        drc.assert_reference_in_range(name, layout, gX, gG, gname, wkind=ftype)
        x, gy, _ = drc.scaled_inputs(name, layout, gX, gG)
        xd = torch.from_numpy(x).to(dev).requires_grad_(True)
        y = conv(xd, edges, sten)
        grads = torch.autograd.grad(y, [xd] + list(conv.parameters()), grad_outputs=torch.from_numpy(gy).to(dev))
        y_ref, gx_ref, gW_ref = drc.scaled_reference(name, layout, gX, gG, wkind=ftype)
        pref = orc.effective_filter_vjp(gW_ref, z.astype(np.float64), s.astype(np.float64), p.astype(np.float64), ftype, B)
        got = (H(y), H(grads[0]), gW_ref)
        assert np.isfinite(got[0].view(np.float32)).all() and np.isfinite(got[1].view(np.float32)).all()
        ey, egx, _ = drc.errors(name, layout, got, (y_ref, gx_ref, gW_ref))
        ep = {}
        for n, g, r in zip(names, grads[1:], pref):
            assert np.isfinite(H(g)).all(), n
            ep[n] = drc.measured_err(H(g), r)
        print(f'  {name} ftype {ftype} x-gy {gname}: row-wise errors y {ey:.2e} gx {egx:.2e} ' + ' '.join('g_%s %.2e' % kv for kv in ep.items()))
        for key, e in dict(ep, y=ey, gx=egx).items():
            worst[key] = max(worst.get(key, 0.0), e)
    assert worst.pop('y') < TOL and worst.pop('gx') < 5 * TOL and all(e < TOL for e in worst.values()), worst


CONTAINMENT_KERNELS = {'ring4400': ('records', 'ring-major', 'streaming'), 'stream3100': ('records', 'streaming'),
                       'split60': ('records', 'frequency-major', 'edge-split', 'kernel-pair')}


@pytest.mark.parametrize('name', drc.CONTAINMENT_SHAPES)
def test_rows_do_not_leak_into_each_other(name, dev):
    graph = build_graph(name, dev)
    require_kernels(name, graph, CONTAINMENT_KERNELS[name])
    layout = 'random'
    P = drc.perturbed_set(name)
    y_aff, gx_aff = drc.affected_rows(name, P)
    x, gy, W = drc.scaled_inputs(name, layout, 0, 0)
    clean = run_explicit(graph, x, gy, W, dev)
    print(f'  {name}: {P.size} perturbed vertices; unaffected rows: y {(~y_aff).sum()} gx {(~gx_aff).sum()} of {x.shape[0]}')
    for label, value in (('2^40', None), ('inf', np.inf), ('nan', np.nan)):
        # -- x[P] -> y
        xp = x.copy()
        xp[P] = xp[P] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = run_explicit(graph, xp, gy, W, dev)
        assert np.isfinite(got[0][~y_aff].view(np.float32)).all(), label
        assert np.array_equal(got[0][~y_aff], clean[0][~y_aff]), ('y rows without an in-edge from P changed', label)
        if value is None:
            assert np.array_equal(xp, drc.scaled_inputs(name, 'random+xP', 0, 0)[0])
            ref = drc.scaled_reference(name, 'random+xP', 0, 0)
            yn, _ = drc.normalised(name, layout, got[0], got[1])
            yr, _ = drc.normalised(name, layout, ref[0], ref[1])
            ey = drc.measured_err(yn, yr, rows=y_aff)
            print(f'  {name} x[P] * 2^40: affected y rows row-wise {ey:.2e}')
            assert ey < TOL
        # -- gy[P] -> gx
        gp = gy.copy()
        gp[P] = gp[P] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = run_explicit(graph, x, gp, W, dev)
        assert np.isfinite(got[1][~gx_aff].view(np.float32)).all(), label
        assert np.array_equal(got[1][~gx_aff], clean[1][~gx_aff]), ('gx rows without an out-edge into P changed', label)
        if value is None:
            assert np.array_equal(gp, drc.scaled_inputs(name, 'random+gP', 0, 0)[1])
            ref = drc.scaled_reference(name, 'random+gP', 0, 0)
            _, gn = drc.normalised(name, layout, got[0], got[1])
            _, gr = drc.normalised(name, layout, ref[0], ref[1])
            eg = drc.measured_err(gn, gr, rows=gx_aff)
            print(f'  {name} gy[P] * 2^40: affected gx rows row-wise {eg:.2e}')
            assert eg < 5 * TOL
