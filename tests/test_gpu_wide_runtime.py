"""The two FieldConv routes that run in pieces, ROW BY ROW against the complex128 oracle (cases: _wide_runtime_cases.py on the
generator of _dynamic_range_cases.py, pinned on the CPU by test_wide_runtime_host.py).

The wide path (csrc/fc_wide.hip, _WideFieldConvFn) runs a layer of more than one channel block as nob x nib launches of the ordinary
kernels: a one-channel tail block (rows of 8 bytes), exact multiples of the block (one output block: gx written without the sum of
parts), a block narrower than 64, the edge split and generic records inside block launches, dense rows, and the three filter types
of the parameter path.  The run-time path (csrc/fc_generic.hip + csrc/fc_cgemm.hip, _GenericFieldConvFn) at the sizes where it
changes shape: the k split of the filter-gradient GEMM, the LDS-sized channel blocks of the double-precision gather, band limit 0.
A relative error of 1e-4 confined to one channel of 129 passes a 1e-5 gate on the global maximum; here x and gy rows, filter rows and
filter columns differ by powers of two under global exponents near both ends of the fp32 range, and every row is measured.

Beyond accuracy: the glue of the wide path is EXACTLY the blocks (bit for bit against the single-block route), rows and channel
blocks do not leak into each other (times 2^40, inf, NaN: values, not faults), and fc_cgemm is measured by rows and by columns, twice
for bit equality.  The route is asserted in every case, from the autograd node and the library's own account.

Gates (the project's: test_gpu_dynamic_range.py, test_gpu_parity.py): wide path complex64 y < TOL, gx < 5 TOL, gW and parameter
gradients < TOL (TOL = 1e-5, or 5e-3 under FC_MFMA=f16); run-time path and fc_cgemm complex64 1e-5 / 5e-5 / 1e-5 whatever FC_MFMA
says; complex128 1e-12 throughout.

Worst row-wise errors measured on an MI355X (default mode), per case over its layouts and global pairs; every case passed, the glue
(c) and both containments (d) bit for bit:
    wide path, explicit filter               y         gx        gW
      wide129 (geometric records)            5.05e-07  3.58e-07  3.16e-07
      wide129 (generic records)              4.48e-07  3.58e-07  3.16e-07
      wide129 (dense rows)                   4.96e-07  4.19e-07  4.00e-07
      wide128                                6.91e-07  4.59e-07  3.00e-07
      wide_narrow_block (block 56)           7.85e-07  4.92e-07  2.96e-07
      wide_split60                           6.96e-07  4.17e-07  4.01e-07
      wide129, x[P] / gy[P] * 2^40           2.83e-07  3.27e-07            (affected rows)
    wide path, parameters                    y         gx        g_zonal   g_spherical  g_phase
      wide129 ftype 0                        5.51e-07  3.71e-07  2.61e-07  3.11e-07
      wide129 ftype 1                        5.22e-07  4.15e-07  2.77e-07  3.16e-07     7.23e-07
      wide129 ftype 2                        4.25e-07  4.46e-07  2.51e-07  3.44e-07
      wide_narrow_block ftype 1              8.58e-07  4.63e-07  2.68e-07  3.19e-07     4.28e-07
    run-time path, explicit filter           y         gx        gW        (complex64 | complex128)
      rt_rings9                              1.32e-06  5.70e-07  5.30e-07  |  3.18e-15  9.51e-16  1.79e-15
      rt_band0                               3.84e-07  2.58e-07  3.35e-07  |  7.44e-16  7.35e-16  5.65e-16
      rt_blocks_f64                          9.14e-07  6.13e-07  4.41e-07  |  2.25e-15  1.69e-15  1.27e-15
      rt_ksplit                              9.16e-07  3.92e-07  6.29e-07  |  1.89e-15  1.00e-15  2.17e-15
    run-time path, parameters (rt_rings9)    y         gx        g_zonal   g_spherical  g_phase
      ftype 1 complex64                      1.14e-06  4.62e-07  4.99e-07  5.08e-07     1.35e-06
      ftype 1 complex128                     3.82e-15  9.86e-16  2.14e-15  3.04e-15     3.61e-15
      ftype 2 complex64                      1.34e-06  4.53e-07  5.14e-07  5.98e-07
      ftype 2 complex128                     3.33e-15  1.19e-15  2.25e-15  2.25e-15
    fc_cgemm, worse of rows and columns      y         gC        gW        (complex64 | complex128)
      (5, 162, 2100), gW split along k       1.08e-06  2.16e-07  1.10e-06  |  1.73e-15  4.32e-16  3.21e-15
      (1, 1, 2049), gW split along k         9.39e-08  9.62e-08  1.73e-07  |  0         0         2.83e-15
      (65, 64, 16)                           6.77e-07  1.95e-06  3.13e-07  |  9.64e-16  2.09e-15  8.60e-16
      (70, 333, 130)                         1.34e-06  6.31e-07  7.28e-07  |  1.77e-15  1.42e-15  2.24e-15
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import _dynamic_range_cases as drc
import _wide_runtime_cases as wrc
from oracle import fieldconv_oracle as orc

pytestmark = pytest.mark.gpu
REDUCED = os.environ.get('FC_MFMA') == 'f16'
TOL = 5e-3 if REDUCED else 1e-5
WIDE_GATES = (TOL, 5 * TOL, TOL)                # y, gx, gW / parameter gradients
RT_GATES = {torch.complex64: (1e-5, 5e-5, 1e-5), torch.complex128: (1e-12, 1e-12, 1e-12)}


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def build_graph(name, dev, dtype=torch.complex64):
    from fieldconv_amd.graph import SupportGraph
    edges, sten = drc.mesh(name)[:2]
    return SupportGraph(torch.from_numpy(edges).to(dev), torch.from_numpy(sten).to(dtype).to(dev), drc.dims(name)[0])


def switches():
    from fieldconv_amd import _env
    return {k: v for k, v in _env.active().items() if k not in ('FIELDCONV_NO_GEO',)}         # (that one is a case of this module)


def node_of(y):
    return type(y.grad_fn).__name__


def check_node(y, node):
    """The autograd node that made y is the route under test -- or skip, with the reason, when a development switch has redirected it."""
    if node_of(y) != node and switches():
        pytest.skip('%s instead of %s under %s' % (node_of(y), node, switches()))
    assert node_of(y) == node, (node_of(y), node)


def describe(graph, I, O, B):
    """The library's own account of the kernels a single launch with these dims takes (fc_describe_kernels)."""
    from fieldconv_amd import _lib
    from fieldconv_amd.functional import make_dims
    kind = 2 if getattr(graph, 'geo_t', None) is not None else (1 if graph.factored else 0)
    buf = ctypes.create_string_buffer(1024)
    assert _lib.load().fc_describe_kernels(ctypes.byref(make_dims(graph, I, O, B)), kind, buf, len(buf)) == 0
    return buf.value.decode()


def require_wide(name, graph, y=None):
    """The block the library picks for this stencil shape; asserts that the layer is wider than it -- and, given an output, that the
    wide node made it.  Under a development switch that changes the block so that the case loses its point: skip, with the reason."""
    from fieldconv_amd.functional import _channel_block
    N, k, I, O, B, R = drc.dims(name)
    blk = _channel_block(graph, I, O, B)
    print('%s %s: channel block %d, %d x %d blocks (out x in), tails %d / %d; %s' % (
        name, drc.dims(name), blk, len(wrc.blocks(O, blk)), len(wrc.blocks(I, blk)), wrc.blocks(O, blk)[-1][1], wrc.blocks(I, blk)[-1][1],
        'records (%s)' % ('geometric' if graph.geo_t is not None else 'generic') if graph.factored else 'dense rows'))
    expect = {'wide129': blk == 64, 'wide129dense': blk == 64, 'wide128': blk == 64, 'wide_narrow_block': blk < 64, 'wide_split60': blk == 64}[name]
    if not expect and (switches() or os.environ.get('FC_MFMA')):
        pytest.skip('%s: channel block %d under %s' % (name, blk, dict(switches(), FC_MFMA=os.environ.get('FC_MFMA'))))
    assert expect, (name, blk)
    assert I > blk, (name, I, blk)
    if y is not None:
        check_node(y, '_WideFieldConvFnBackward')
    return blk


def require_run_time(name, dtype, y=None):
    from fieldconv_amd import _lib
    N, k, I, O, B, R = drc.dims(name)
    assert dtype == torch.complex128 or _lib.load().fc_shape_compiled(R, B) == 0, (name, R, B)
    if y is not None:
        assert y.dtype == dtype
        check_node(y, '_GenericFieldConvFnBackward')


def run_explicit(graph, x, gy, W, dev, dtype=torch.complex64, node=None):
    from fieldconv_amd.functional import field_conv
    xd = torch.from_numpy(x).to(dtype).to(dev).requires_grad_(True)
    Wd = torch.from_numpy(W).to(dtype).to(dev).requires_grad_(True)
    y = field_conv(xd, Wd, graph)
    if node is not None:
        check_node(y, node)
    gx, gW = torch.autograd.grad(y, [xd, Wd], grad_outputs=torch.from_numpy(gy).to(dtype).to(dev))
    return H(y), H(gx), H(gW)


def finite(t):
    return bool(np.isfinite(t).all())                 # (complex: both parts)


def block_breakdown(name, layout, got, ref, blk):
    """The measure of drc.errors per output block (y), per input block (gx) and per (output block, input block) (gW)."""
    N, k, I, O, B, R = drc.dims(name)
    yn, gxn = drc.normalised(name, layout, got[0], got[1])
    yr, gxr = drc.normalised(name, layout, ref[0], ref[1])
    lines = []
    for ob, (o0, bo) in enumerate(wrc.blocks(O, blk)):
        lines.append('y[:, ob %d] %.2e' % (ob, drc.measured_err(yn[:, o0:o0 + bo], yr[:, o0:o0 + bo])))
    for ib, (i0, bi) in enumerate(wrc.blocks(I, blk)):
        lines.append('gx[:, ib %d] %.2e' % (ib, drc.measured_err(gxn[:, i0:i0 + bi], gxr[:, i0:i0 + bi])))
    for ob, (o0, bo) in enumerate(wrc.blocks(O, blk)):
        for ib, (i0, bi) in enumerate(wrc.blocks(I, blk)):
            lines.append('gW[ob %d, ib %d] %.2e' % (ob, ib, drc.measured_err(got[2][o0:o0 + bo, i0:i0 + bi], ref[2][o0:o0 + bo, i0:i0 + bi])))
    return '; '.join(lines)


# ---------------------------------------------------------------- a. row-wise accuracy, wide path
WIDE_CASES = [
    pytest.param('wide129', False, id='wide129'),
    pytest.param('wide129', True, id='wide129-generic-records'),
    pytest.param('wide129dense', False, id='wide129-dense-rows'),
    pytest.param('wide128', False, id='wide128'),
    pytest.param('wide_narrow_block', False, id='wide-narrow-block'),
    pytest.param('wide_split60', False, id='wide-split60'),
]


@pytest.mark.parametrize('layout', drc.LAYOUTS)
@pytest.mark.parametrize('name,no_geo', WIDE_CASES)
def test_wide_path_rowwise(name, no_geo, layout, dev, monkeypatch):
    if no_geo:
        monkeypatch.setenv('FIELDCONV_NO_GEO', '1')
    graph = build_graph(name, dev)
    blk = require_wide(name, graph)
    if name == 'wide129dense':
        assert not graph.factored and graph.sten_t is not None
    else:
        assert graph.factored and (not no_geo or graph.geo_t is None)
    if name == 'wide_split60':            # the block launches of this mesh take the edge split, the full block and the tails alike
        import re
        N, k, I, O, B, R = drc.dims(name)
        for bi, bo in ((blk, blk), (wrc.blocks(I, blk)[-1][1], wrc.blocks(O, blk)[-1][1])):
            desc = describe(graph, bi, bo, B)
            parts = re.search(r'parts=(\d+)', desc.split(';', 1)[0])
            if (parts is None or int(parts.group(1)) <= 1) and switches():
                pytest.skip('no edge split under %s: %s' % (switches(), desc))
            assert parts is not None and int(parts.group(1)) > 1, desc
            print('  block launch %d -> %d: %s' % (bi, bo, desc))
    worst, report = [0.0, 0.0, 0.0], []
    for gname in wrc.WIDE_GLOBALS:
        gX, gG = drc.GLOBALS[gname]
        drc.assert_reference_in_range(name, layout, gX, gG, gname)
        got = run_explicit(graph, *drc.scaled_inputs(name, layout, gX, gG), dev, node='_WideFieldConvFnBackward')
        ref = drc.scaled_reference(name, layout, gX, gG)
        assert all(finite(t) for t in got), (name, layout, gname)
        errs = drc.errors(name, layout, got, ref)
        print('  %s %s x-gy %s: row-wise errors y %.2e gx %.2e gW %.2e' % ((name, layout, gname) + errs))
        if not all(e < g for e, g in zip(errs, WIDE_GATES)):
            report.append('%s: %s' % (gname, block_breakdown(name, layout, got, ref, blk)))
            print('  per block, ' + report[-1])
        worst = [max(w, e) for w, e in zip(worst, errs)]
    assert all(w < g for w, g in zip(worst, WIDE_GATES)), (worst, report)


# ---------------------------------------------------------------- b. parameter path, wide; and on the run-time path (e)
def run_module(name, ftype, layout, globals_, gates, dev, dtype, node):
    from fieldconv_amd.nn import FieldConv
    N, k, I, O, B, R = drc.dims(name)
    real = torch.float64 if dtype == torch.complex128 else torch.float32
    edges, sten = drc.mesh(name)[:2]
    edges, sten = torch.from_numpy(edges).to(dev), torch.from_numpy(sten).to(dtype).to(dev)
    z, s, p = drc.scaled_params(name, layout, ftype)
    conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=ftype)
    conv.load_state_dict({'zonal': torch.from_numpy(z), 'spherical': torch.from_numpy(s), 'phase': torch.from_numpy(p)})
    conv = conv.to(real).to(dev)
    names = [n for n, _ in conv.named_parameters()]
    assert names == ['zonal', 'spherical', 'phase'][:len(names)]
    worst = {}
    for gname in globals_:
        gX, gG = drc.GLOBALS[gname]
        drc.assert_reference_in_range(name, layout, gX, gG, gname, wkind=ftype)
        x, gy, _ = drc.scaled_inputs(name, layout, gX, gG)
        xd = torch.from_numpy(x).to(dtype).to(dev).requires_grad_(True)
        y = conv(xd, edges, sten)
        check_node(y, node)
        assert y.dtype == dtype, y.dtype
        grads = torch.autograd.grad(y, [xd] + list(conv.parameters()), grad_outputs=torch.from_numpy(gy).to(dtype).to(dev))
        y_ref, gx_ref, gW_ref = drc.scaled_reference(name, layout, gX, gG, wkind=ftype)
        pref = orc.effective_filter_vjp(gW_ref, z.astype(np.float64), s.astype(np.float64), p.astype(np.float64), ftype, B)
        got = (H(y), H(grads[0]), gW_ref)
        assert finite(got[0]) and finite(got[1])
        ey, egx, _ = drc.errors(name, layout, got, (y_ref, gx_ref, gW_ref))
        ep = {}
        for n, g, r in zip(names, grads[1:], pref):
            assert g.dtype == real and np.isfinite(H(g)).all(), n
            ep[n] = drc.measured_err(H(g), r)
        print('  %s ftype %d %s x-gy %s: row-wise errors y %.2e gx %.2e ' % (name, ftype, str(dtype)[6:], gname, ey, egx)
              + ' '.join('g_%s %.2e' % kv for kv in ep.items()))
        for key, e in dict(ep, y=ey, gx=egx).items():
            worst[key] = max(worst.get(key, 0.0), e)
    w = dict(worst)
    assert w.pop('y') < gates[0] and w.pop('gx') < gates[1] and all(e < gates[2] for e in w.values()), worst


@pytest.mark.parametrize('name,ftype', wrc.WIDE_PARAM_CASES, ids=['%s-ftype%d' % c for c in wrc.WIDE_PARAM_CASES])
def test_wide_parameter_path(name, ftype, dev):
    """zonal / spherical rows and columns scaled by the powers of two of the explicit filter: filter images packed from the (o0, i0)
    block of the parameter tensors, parameter gradients landing in their block; against the oracle's chain rule, row-wise."""
    require_wide(name, build_graph(name, dev))
    run_module(name, ftype, 'random', wrc.WIDE_GLOBALS, WIDE_GATES, dev, torch.complex64, '_WideFieldConvFnBackward')


# ---------------------------------------------------------------- c. the glue is exactly the blocks
@pytest.mark.parametrize('name', ['wide129', 'wide_split60'])
def test_wide_glue_is_exactly_the_blocks(name, dev):
    """The wide call against one single-block call (_FieldConvFn) per (output block, input block) on the cut inputs, bit for bit:
      y[:, ob]   = fp32 sum over ib, in block order, of the block outputs: ((y_0 + y_1) + y_2) -- the sum rides in the residual
                   epilogue of launch ib > 0 (addend: the output block so far), which is bit-identical to the separate add;
      gW[ob, ib] = the single-block gW;
      gx[:, ib]  = fp32 sum over ob, in block order, of the block input gradients: fc_sum_parts_kernel starts from part 0 and adds
                   parts 1, 2, ... left to right (csrc/fc_tile.hpp)."""
    from fieldconv_amd.functional import field_conv
    graph = build_graph(name, dev)
    blk = require_wide(name, graph)
    N, k, I, O, B, R = drc.dims(name)
    x, gy, W = (torch.from_numpy(t).to(dev) for t in drc.scaled_inputs(name, 'random', 0, 0))
    xw, Ww = x.clone().requires_grad_(True), W.clone().requires_grad_(True)
    y = field_conv(xw, Ww, graph)
    check_node(y, '_WideFieldConvFnBackward')
    gx, gW = torch.autograd.grad(y, [xw, Ww], grad_outputs=gy)
    ysum = {}
    gxsum = {}
    for ob, (o0, bo) in enumerate(wrc.blocks(O, blk)):
        for ib, (i0, bi) in enumerate(wrc.blocks(I, blk)):
            xb = x[:, i0:i0 + bi].contiguous().requires_grad_(True)
            Wb = W[o0:o0 + bo, i0:i0 + bi].contiguous().requires_grad_(True)
            yb = field_conv(xb, Wb, graph)
            check_node(yb, '_FieldConvFnBackward')
            gxb, gWb = torch.autograd.grad(yb, [xb, Wb], grad_outputs=gy[:, o0:o0 + bo].contiguous())
            ysum[ob] = yb.detach() if ib == 0 else ysum[ob] + yb.detach()
            gxsum[ib] = gxb if ob == 0 else gxsum[ib] + gxb
            assert torch.equal(gW[o0:o0 + bo, i0:i0 + bi], gWb), ('gW block', ob, ib)
    for ob, (o0, bo) in enumerate(wrc.blocks(O, blk)):
        assert torch.equal(y[:, o0:o0 + bo], ysum[ob]), ('y block', ob, float((y[:, o0:o0 + bo] - ysum[ob]).abs().max()))
    for ib, (i0, bi) in enumerate(wrc.blocks(I, blk)):
        assert torch.equal(gx[:, i0:i0 + bi], gxsum[ib]), ('gx block', ib, float((gx[:, i0:i0 + bi] - gxsum[ib]).abs().max()))


# ---------------------------------------------------------------- d. containment
def test_wide_rows_do_not_leak_into_each_other(dev):
    """test_gpu_dynamic_range.py::test_rows_do_not_leak_into_each_other on wide129."""
    name, layout = 'wide129', 'random'
    graph = build_graph(name, dev)
    require_wide(name, graph)
    P = drc.perturbed_set(name)
    y_aff, gx_aff = drc.affected_rows(name, P)
    x, gy, W = drc.scaled_inputs(name, layout, 0, 0)
    clean = run_explicit(graph, x, gy, W, dev, node='_WideFieldConvFnBackward')
    print('  %s: %d perturbed vertices; unaffected rows: y %d gx %d of %d' % (name, P.size, (~y_aff).sum(), (~gx_aff).sum(), x.shape[0]))
    for label, value in (('2^40', None), ('inf', np.inf), ('nan', np.nan)):
        xp = x.copy()
        xp[P] = xp[P] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = run_explicit(graph, xp, gy, W, dev)
        assert finite(got[0][~y_aff]), label
        assert np.array_equal(got[0][~y_aff], clean[0][~y_aff]), ('y rows without an in-edge from P changed', label)
        if value is None:
            ref = drc.scaled_reference(name, 'random+xP', 0, 0)
            yn, _ = drc.normalised(name, layout, got[0], got[1])
            yr, _ = drc.normalised(name, layout, ref[0], ref[1])
            ey = drc.measured_err(yn, yr, rows=y_aff)
            print('  %s x[P] * 2^40: affected y rows row-wise %.2e' % (name, ey))
            assert ey < TOL
        gp = gy.copy()
        gp[P] = gp[P] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        got = run_explicit(graph, x, gp, W, dev)
        assert finite(got[1][~gx_aff]), label
        assert np.array_equal(got[1][~gx_aff], clean[1][~gx_aff]), ('gx rows without an out-edge into P changed', label)
        if value is None:
            ref = drc.scaled_reference(name, 'random+gP', 0, 0)
            _, gn = drc.normalised(name, layout, got[0], got[1])
            _, gr = drc.normalised(name, layout, ref[0], ref[1])
            eg = drc.measured_err(gn, gr, rows=gx_aff)
            print('  %s gy[P] * 2^40: affected gx rows row-wise %.2e' % (name, eg))
            assert eg < 5 * TOL


def test_wide_channel_blocks_do_not_leak_into_each_other(dev):
    """Input block 1 of x poisoned: gx[:, ib] and gW[:, ib] of the other input blocks are sums over launches that never read it.
    Filter rows of output block 1 poisoned: y[:, block 0] and gW[block 0] never read them.  Bit-identical and finite."""
    name = 'wide129'
    graph = build_graph(name, dev)
    blk = require_wide(name, graph)
    N, k, I, O, B, R = drc.dims(name)
    (i0, bi), (o0, bo) = wrc.blocks(I, blk)[1], wrc.blocks(O, blk)[1]
    x, gy, W = drc.scaled_inputs(name, 'random', 0, 0)
    clean = run_explicit(graph, x, gy, W, dev)
    other_i = np.ones(I, bool)
    other_i[i0:i0 + bi] = False
    for label, value in (('2^40', None), ('inf', np.inf), ('nan', np.nan)):
        xp = x.copy()
        xp[:, i0:i0 + bi] = xp[:, i0:i0 + bi] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        _, gx, gW = run_explicit(graph, xp, gy, W, dev)
        assert finite(gx[:, other_i]) and finite(gW[:, other_i]), label
        assert np.array_equal(gx[:, other_i], clean[1][:, other_i]), ('gx columns outside input block 1 changed', label)
        assert np.array_equal(gW[:, other_i], clean[2][:, other_i]), ('gW columns outside input block 1 changed', label)
        Wp = W.copy()
        Wp[o0:o0 + bo] = Wp[o0:o0 + bo] * np.float32(2.0 ** drc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
        y, _, gW = run_explicit(graph, x, gy, Wp, dev)
        assert finite(y[:, :o0]) and finite(gW[:o0]), label
        assert np.array_equal(y[:, :o0], clean[0][:, :o0]), ('y columns of output block 0 changed', label)
        assert np.array_equal(gW[:o0], clean[2][:o0]), ('gW rows of output block 0 changed', label)


# ---------------------------------------------------------------- e. row-wise accuracy, run-time path
@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128], ids=['c64', 'c128'])
@pytest.mark.parametrize('name', list(wrc.RT_SHAPES))
def test_run_time_path_rowwise(name, dtype, dev):
    """Explicit filter, layout random; the complex128 inputs are the complex64 ones widened, so one reference serves both."""
    from fieldconv_amd import _lib
    N, k, I, O, B, R = drc.dims(name)
    F = 2 * B + 1
    layout = 'random'
    require_run_time(name, dtype)
    dt = 1 if dtype == torch.complex128 else 0
    if name == 'rt_ksplit':
        with torch.cuda.device(dev):
            assert _lib.load().fc_cgemm_workspace_bytes(O, I * R * F, N, dt) > 0            # the filter-gradient product goes split along k
    if name == 'rt_blocks_f64':
        assert len(wrc.blocks(I, min(I, wrc.gather_block(R, F, 16 if dt else 8)))) == (2 if dt else 1)
    graph = build_graph(name, dev, dtype)
    assert not graph.factored and graph.sten_t is not None and graph.sten_t.dtype == dtype
    gates = RT_GATES[dtype]
    worst = [0.0, 0.0, 0.0]
    for gname in wrc.RT_GLOBALS:
        gX, gG = drc.GLOBALS[gname]
        drc.assert_reference_in_range(name, layout, gX, gG, gname)
        got = run_explicit(graph, *drc.scaled_inputs(name, layout, gX, gG), dev, dtype=dtype, node='_GenericFieldConvFnBackward')
        assert all(t.dtype == (np.complex128 if dt else np.complex64) and finite(t) for t in got), (name, gname)
        errs = drc.errors(name, layout, got, drc.scaled_reference(name, layout, gX, gG))
        print('  %s %s x-gy %s: row-wise errors y %.2e gx %.2e gW %.2e' % ((name, str(dtype)[6:], gname) + errs))
        worst = [max(w, e) for w, e in zip(worst, errs)]
    assert all(w < g for w, g in zip(worst, gates)), worst


@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128], ids=['c64', 'c128'])
@pytest.mark.parametrize('name,ftype', wrc.RT_PARAM_CASES, ids=['%s-ftype%d' % c for c in wrc.RT_PARAM_CASES])
def test_run_time_parameter_path(name, ftype, dtype, dev):
    require_run_time(name, dtype)
    run_module(name, ftype, 'random', wrc.RT_GLOBALS, RT_GATES[dtype], dev, dtype, '_GenericFieldConvFnBackward')


# ---------------------------------------------------------------- f. fc_cgemm by rows and by columns
@pytest.mark.parametrize('dtype', [torch.complex64, torch.complex128], ids=['c64', 'c128'])
@pytest.mark.parametrize('size', wrc.CGEMM_SIZES, ids=lambda s: 'O%d_K%d_n%d' % s)
def test_cgemm_rows_and_columns(size, dtype, dev):
    """The three layouts of test_gpu_parity.py::test_cgemm_three_layouts with the rows of A and G scaled by powers of two, measured
    row-wise and column-wise against the complex128 product; each product twice, bit-equal (the k-split reduction is order-fixed)."""
    from fieldconv_amd import _lib
    from fieldconv_amd.functional import _cgemm
    lib = _lib.load()
    O, K, n = size
    dt = 1 if dtype == torch.complex128 else 0
    gate = RT_GATES[dtype][0]
    c = wrc.cgemm_case(O, K, n)
    with torch.cuda.device(dev):
        split = lib.fc_cgemm_workspace_bytes(O, K, n, dt) > 0
    assert split == (n >= 2048), (size, split)
    A, W, G = (torch.from_numpy(c[key].copy()).to(dtype).to(dev) for key in ('A', 'W', 'G'))
    products = {            # C shape, (A, B, M, N, K, sam, sak, sbk, sbn, conj_b, alpha)
        'y': ((n, O), (A, W, n, O, K, K, 1, 1, K, False, 0.5)),
        'gC': ((n, K), (G, W, n, K, O, O, 1, K, 1, True, 1.0)),
        'gW': ((O, K), (G, A, O, K, n, 1, O, K, 1, True, 2.0)),
    }
    for key, (shape, (a, b, *rest)) in products.items():
        outs = []
        for _ in range(2):
            out = torch.full(shape, float('nan'), dtype=dtype, device=dev)
            _cgemm(lib, a, b, out, *rest)
            outs.append(H(out))
        assert finite(outs[0]) and np.array_equal(outs[0], outs[1]), (key, 'two runs differ')
        er, ec = wrc.rows_and_columns_err(outs[0], c['ref'][key])
        print('  cgemm %s %s %s%s: row-wise %.2e column-wise %.2e' % (size, str(dtype)[6:], key, ' (k split)' if split and key == 'gW' else '', er, ec))
        assert er < gate and ec < gate, (key, er, ec)
