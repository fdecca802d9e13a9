"""Pins the inputs of the pointwise-operator tests (_pointwise_cases.py) and the route account of the TangentLin launchers
(fc_tangent_lin_describe) on the CPU, so that test_gpu_pointwise.py cannot hide a failure behind its own inputs or gates:

  * the scaled inputs are exact in fp32, every 16-row block spans the exponent ranges, the origin box holds the exact zeros and
    the planted entries only, no modReLU gate is decided by rounding, and no reference row but the planted one is zero;
  * the same products and sums in plain fp32 numpy stay below a QUARTER of the GPU gate (1e-5, test_gpu_parity.py's TOL in the
    default mode) by the same measures -- row-wise for y and gx, global for the parameter gradients: the gate does not fail a
    correct fp32 kernel on these inputs;
  * every TangentLin case takes, at the 256 compute units the library assumes without a device, the route it is named for."""
import ctypes

import numpy as np
import pytest

import _pointwise_cases as pc
from conftest import rel_err

GATE = 1e-5                     # tests/test_gpu_parity.py: TOL without FC_MFMA=f16
CASES = pc.lin_cases(pc.DEFAULT_CUS)
LIN_SHAPES = sorted({(c.N, c.I, c.O) for c in CASES.values()})
NONLIN_ALL = pc.NONLIN_SHAPES + pc.NONLIN_F64_SHAPES


def test_case_tables_are_what_the_issue_lists():
    assert pc.LIN_NAMES == tuple(CASES) and len(CASES) == 17 + 8 and set(pc.CONTAINMENT_NAMES) <= set(CASES)
    c = pc.DEFAULT_CUS
    assert CASES['split-trip2'].N == 16427 and CASES['unsplit-4tiles'].N == 32789 and CASES['unsplit-trip2'].N == 65543
    assert CASES['direct-trip2'].N == 16393 and c == 256
    assert sorted(n for n in CASES if CASES[n].offset) == ['lds-misaligned', 'misaligned-trip2']


@pytest.mark.parametrize('N', sorted({s[0] for s in LIN_SHAPES} | {s[0] for s in NONLIN_ALL}))
def test_every_block_spans_the_exponent_ranges(N):
    a, d = pc.exponents(N)
    special = np.zeros(N, bool)
    special[pc.special_rows(N)] = True
    assert np.all(a[special] == pc.A_RANGE[0]) and not special[::pc.BLOCK][1:].any()
    for e, (lo, hi) in ((a, pc.A_RANGE), (d, pc.D_RANGE)):
        assert e.min() >= lo and e.max() <= hi
        for b in range(0, N, pc.BLOCK):
            blk = e[b:b + pc.BLOCK]
            if blk.size >= 2:
                assert blk.min() == lo, (N, b)
                assert blk.max() == hi or (e is a and special[b]), (N, b)
    if N > 64:                  # random inside a block, not a pattern
        assert len(set(map(tuple, a[:N // pc.BLOCK * pc.BLOCK].reshape(-1, pc.BLOCK)))) > 1
    P = pc.perturbed_rows(N)
    assert P[-1] == N - 1 and np.all(P[:-1] % pc.BLOCK == pc.BLOCK - 1) and (N < 112 or P.size >= 2)


@pytest.mark.parametrize('N,I,O', LIN_SHAPES + [(n, c, c) for n, c in NONLIN_ALL] + [pc.GEMM_F64_CASE])
def test_scaled_inputs_are_exact_in_fp32(N, I, O):
    x0, gy0, Re, Im, bias = pc.base(N, I, O)
    x, gy = pc.inputs(N, I, O)[:2]
    a, d = pc.exponents(N)
    for t, t0, e in ((x, x0, a), (gy, gy0, d)):
        assert t.dtype == np.complex64 and np.isfinite(t.view(np.float32)).all()
        assert np.array_equal(t.astype(np.complex128), t0.astype(np.complex128) * np.ldexp(1.0, e)[:, None])
    assert Re.dtype == Im.dtype == bias.dtype == np.float32 and bias.shape == (1, I) and bias[0, 0] > 0 and (I == 1 or bias[0, 1] < 0)
    z = pc.zero_row(N)
    assert (z is None) == (N < 3) and (z is None or not x[z].any())
    if N * I >= 100:
        assert (x0 == 0).sum() > (I if z is not None else 0)              # exact zeros beyond the zero row
    box = pc.origin_box(x)
    mag = np.maximum(np.abs(x.real), np.abs(x.imag))
    assert mag[box].max(initial=0.0) < 0.7e-7 and mag[~box].min(initial=1.0) > 1.15e-7
    pc.assert_box_is_the_planted_set(N, I, O)
    assert len(pc.planted(N, I)) == (0 if N * I < 4 else 3)


@pytest.mark.parametrize('N,I,O', LIN_SHAPES)
def test_lin_conditions_and_fp32_pin(N, I, O):
    pc.assert_lin_conditions(N, I, O)
    x, gy, Re, Im, _ = pc.inputs(N, I, O)
    y_ref, gx_ref, gRe_ref, gIm_ref = pc.lin_reference(N, I, O)
    Wc = (Re + 1j * Im).astype(np.complex64)
    y, gx, gW = x @ Wc.T, gy @ np.conj(Wc), gy.T @ np.conj(x)
    assert y.dtype == gx.dtype == gW.dtype == np.complex64
    errs = (pc.rowwise_err(y, y_ref), pc.rowwise_err(gx, gx_ref), rel_err(gW.real, gRe_ref), rel_err(gW.imag, gIm_ref))
    print('fp32 numpy (%d, %d, %d): y %.2e gx %.2e gRe %.2e gIm %.2e' % ((N, I, O) + errs))
    assert max(errs) < GATE / 4, errs


def _modrelu_fp32(x, gy, bias):
    """The modReLU and its VJP in plain fp32 numpy, operation by operation."""
    f32 = np.float32
    vx, vy, gx_, gy_ = x.real, x.imag, gy.real, gy.imag
    box = pc.origin_box(x)
    with np.errstate(all='ignore'):
        rad = np.sqrt(vx * vx + vy * vy)
        rad = np.where(box, f32(1), rad)
        f = np.maximum(rad + bias, f32(0))
        s = f / rad
        y = np.where(box, x, (vx * s) + 1j * (vy * s)).astype(np.complex64)
        inv = f32(1) / rad
        ex, ey = vx * inv, vy * inv
        g_rad, g_tan = gx_ * ex + gy_ * ey, gy_ * ex - gx_ * ey
        act = (rad + bias) > 0
        fr = np.where(act, g_rad, f32(0))
        ft = np.where(act, rad + bias, f32(0)) * inv * g_tan
        gx = np.where(box, gy, (ex * fr - ey * ft) + 1j * (ey * fr + ex * ft)).astype(np.complex64)
        gb = np.where(box, f32(0), fr).sum(axis=0, dtype=f32)
    assert rad.dtype == s.dtype == ft.dtype == gb.dtype == f32
    return y, gx, gb


@pytest.mark.parametrize('N,C', pc.NONLIN_SHAPES)
def test_nonlin_conditions_and_fp32_pin(N, C):
    pc.assert_nonlin_conditions(N, C)
    x, gy, _, _, bias = pc.inputs(N, C, C)
    y_ref, gx_ref, gb_ref = pc.nonlin_reference(N, C)
    y, gx, gb = _modrelu_fp32(x, gy, bias)
    box = pc.origin_box(x)
    assert np.array_equal(y_ref[box], x[box]) and np.array_equal(gx_ref[box], gy[box])
    errs = [pc.rowwise_err(y, y_ref), pc.rowwise_err(gx, gx_ref), rel_err(gb.reshape(-1), gb_ref.reshape(-1))]
    sy_ref, sgx_ref = pc.soft_abs_reference(N, C)
    with np.errstate(all='ignore'):
        r = np.sqrt(x.real * x.real + x.imag * x.imag)
        sy = np.where(box, np.float32(0), r)
        s = gy.real / np.where(box, np.float32(1), r)
        sgx = np.where(box, 0, x.real * s + 1j * (x.imag * s)).astype(np.complex64)
    assert sy.dtype == np.float32
    errs += [pc.rowwise_err(sy, sy_ref), pc.rowwise_err(sgx, sgx_ref)]
    print('fp32 numpy (%d, %d): y %.2e gx %.2e gbias %.2e softAbs %.2e / %.2e' % ((N, C) + tuple(errs)))
    assert max(errs) < GATE / 4, errs


@pytest.mark.parametrize('N,C', pc.NONLIN_F64_SHAPES)
def test_nonlin_f64_conditions_and_the_longdouble_restatement(N, C):
    """The longdouble restatement is the oracle's operator: they agree to double precision, by the measures of the GPU test."""
    pc.assert_nonlin_conditions(N, C)
    y_ref, gx_ref, gb_ref = pc.nonlin_reference(N, C)
    (yr, yi), (gr, gi), gb = pc.nonlin_reference_longdouble(N, C)
    assert yr.dtype == np.longdouble and np.finfo(np.longdouble).eps < 1e-18
    y, gx = yr.astype(np.float64) + 1j * yi.astype(np.float64), gr.astype(np.float64) + 1j * gi.astype(np.float64)
    assert pc.rowwise_err(y, y_ref) < 1e-14 and pc.rowwise_err(gx, gx_ref) < 1e-14
    assert rel_err(gb.astype(np.float64).reshape(-1), gb_ref.reshape(-1)) < 1e-13


def test_gemm_f64_case_conditions():
    pc.assert_lin_conditions(*pc.GEMM_F64_CASE)


# ------------------------------------------------------------------ fc_tangent_lin_describe
def _describe(lib, N, K, M, transposed, aligned, size=256):
    buf = ctypes.create_string_buffer(size)
    rc = lib.fc_tangent_lin_describe(N, K, M, transposed, aligned, buf, size)
    return rc, buf.value.decode()


# name -> (forward line, transposed line) at 256 compute units
ROUTES_256 = {
    'split-trip2': ('staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=1024 blocks=1027 trips=2 cus=256',
                    'direct grid=1024 blocks=1027 trips=2 cus=256'),
    'split-trip2-T': ('direct grid=1024 blocks=1027 trips=2 cus=256',
                      'staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=1024 blocks=1027 trips=2 cus=256'),
    'unsplit-4tiles': ('staged split=0 loads=vector tiles=4 kchunks=1 lds=28672 grid=513 blocks=2050 trips=1 cus=256',
                       'staged split=0 loads=vector tiles=2 kchunks=2 lds=30720 grid=513 blocks=2050 trips=1 cus=256'),
    'unsplit-4tiles-T': ('staged split=0 loads=vector tiles=2 kchunks=2 lds=30720 grid=513 blocks=2050 trips=1 cus=256',
                         'staged split=0 loads=vector tiles=4 kchunks=1 lds=28672 grid=513 blocks=2050 trips=1 cus=256'),
    'unsplit-2tiles': ('staged split=0 loads=vector tiles=2 kchunks=1 lds=14336 grid=513 blocks=2050 trips=1 cus=256',
                       'staged split=0 loads=scalar tiles=2 kchunks=1 lds=14336 grid=513 blocks=2050 trips=1 cus=256'),
    'unsplit-trip2': ('staged split=0 loads=vector tiles=3 kchunks=1 lds=15360 grid=1024 blocks=4097 trips=2 cus=256',
                      'staged split=0 loads=vector tiles=1 kchunks=1 lds=11264 grid=1024 blocks=4097 trips=2 cus=256'),
    'scalar-trip2': ('staged split=0 loads=scalar tiles=1 kchunks=1 lds=3072 grid=1024 blocks=4097 trips=2 cus=256',
                     'staged split=0 loads=scalar tiles=1 kchunks=1 lds=3072 grid=1024 blocks=4097 trips=2 cus=256'),
    'misaligned-trip2': ('staged split=0 loads=scalar tiles=1 kchunks=1 lds=5120 grid=1024 blocks=4097 trips=2 cus=256',
                         'staged split=0 loads=scalar tiles=1 kchunks=1 lds=5120 grid=1024 blocks=4097 trips=2 cus=256'),
    'scalar-chunk2': ('staged split=1 loads=scalar tiles=2 kchunks=2 lds=34816 grid=13 blocks=13 trips=1 cus=256',
                      'staged split=1 loads=vector tiles=4 kchunks=1 lds=28672 grid=13 blocks=13 trips=1 cus=256'),
    'scalar-chunk2-T': ('staged split=1 loads=vector tiles=4 kchunks=1 lds=28672 grid=13 blocks=13 trips=1 cus=256',
                        'staged split=1 loads=scalar tiles=2 kchunks=2 lds=34816 grid=13 blocks=13 trips=1 cus=256'),
    'scalar-chunk2-odd': ('staged split=1 loads=scalar tiles=3 kchunks=2 lds=46080 grid=13 blocks=13 trips=1 cus=256',
                          'staged split=1 loads=scalar tiles=4 kchunks=1 lds=45056 grid=13 blocks=13 trips=1 cus=256'),
    'lds-forward': ('staged split=1 loads=vector tiles=4 kchunks=2 lds=69632 grid=13 blocks=13 trips=1 cus=256',
                    'direct grid=13 blocks=13 trips=1 cus=256'),
    'lds-T': ('direct grid=13 blocks=13 trips=1 cus=256',
              'staged split=1 loads=vector tiles=4 kchunks=2 lds=69632 grid=13 blocks=13 trips=1 cus=256'),
    'lds-misaligned': ('staged split=1 loads=scalar tiles=4 kchunks=2 lds=69632 grid=13 blocks=13 trips=1 cus=256',
                       'staged split=1 loads=scalar tiles=4 kchunks=2 lds=69632 grid=13 blocks=13 trips=1 cus=256'),
    'direct-k8': ('direct grid=7 blocks=7 trips=1 cus=256',
                  'staged split=0 loads=scalar tiles=1 kchunks=1 lds=7168 grid=2 blocks=7 trips=1 cus=256'),
    'direct-k64': ('direct grid=7 blocks=7 trips=1 cus=256', 'direct grid=7 blocks=7 trips=1 cus=256'),
    'direct-trip2': ('direct grid=1024 blocks=1025 trips=2 cus=256',
                     'staged split=0 loads=vector tiles=1 kchunks=2 lds=17408 grid=257 blocks=1025 trips=1 cus=256'),
    'edge-staged-N1': ('staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=1 blocks=1 trips=1 cus=256',
                       'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-staged-N15': ('staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=1 blocks=1 trips=1 cus=256',
                        'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-staged-N16': ('staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=1 blocks=1 trips=1 cus=256',
                        'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-staged-N17': ('staged split=1 loads=vector tiles=2 kchunks=1 lds=14336 grid=2 blocks=2 trips=1 cus=256',
                        'direct grid=2 blocks=2 trips=1 cus=256'),
    'edge-direct-N1': ('direct grid=1 blocks=1 trips=1 cus=256', 'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-direct-N15': ('direct grid=1 blocks=1 trips=1 cus=256', 'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-direct-N16': ('direct grid=1 blocks=1 trips=1 cus=256', 'direct grid=1 blocks=1 trips=1 cus=256'),
    'edge-direct-N17': ('direct grid=2 blocks=2 trips=1 cus=256', 'direct grid=2 blocks=2 trips=1 cus=256'),
}


@pytest.fixture(scope='module')
def lib():
    import torch
    from fieldconv_amd import _env, _lib
    if torch.cuda.is_available() and torch.cuda.get_device_properties(0).multi_processor_count != pc.DEFAULT_CUS:
        pytest.skip('the device present has another CU count, which sizes the grids (test_gpu_pointwise.py asserts the routes there)')
    if any(k in _env.LIBRARY_SWITCHES for k in _env.active()):
        pytest.skip('a development switch of the library is set')
    return _lib.load()


@pytest.mark.parametrize('name', pc.LIN_NAMES)
def test_route_of_every_tangent_lin_case_at_256_cus(name, lib):
    case = CASES[name]
    aligned = 0 if case.offset else 1
    rc_f, fwd = _describe(lib, case.N, case.I, case.O, 0, aligned)
    rc_b, bwd = _describe(lib, case.N, case.O, case.I, 1, aligned)
    assert rc_f == 0 and rc_b == 0
    assert (fwd, bwd) == ROUTES_256[name]
    # ... and the pinned lines hold what the case is there for
    assert not pc.route_mismatch(pc.parse_route(fwd), case.fwd), (fwd, case.fwd)
    assert not pc.route_mismatch(pc.parse_route(bwd), case.bwd), (bwd, case.bwd)
    lds = 2 * (-(-case.O // 16) * 16) * (-(-2 * case.I // 16) * 16 + 8) * 4
    assert pc.parse_route(fwd).get('lds', lds) == lds


def test_describe_error_returns_and_abi(lib):
    assert lib.fc_abi_version() == 11
    buf = ctypes.create_string_buffer(256)
    for bad in ((0, 8, 8, 0, 1), (-5, 8, 8, 0, 1), (10, 0, 8, 0, 1), (10, 8, 0, 1, 1), (10, 8, 8, 2, 1), (10, 8, 8, 0, 2), (10, 8, 8, -1, 0),
                (10, 200, 200, 0, 1)):           # (the last: more LDS than a CU has -- the launchers refuse it)
        assert lib.fc_tangent_lin_describe(*bad, buf, len(buf)) == -1, bad
    assert lib.fc_tangent_lin_describe(10, 8, 8, 0, 1, None, 256) == -1
    assert lib.fc_tangent_lin_describe(10, 8, 8, 0, 1, buf, 1) == -1
    rc, line = _describe(lib, 100, 64, 64, 0, 1)
    assert rc == 0 and line == 'direct grid=7 blocks=7 trips=1 cus=256'
    small = ctypes.create_string_buffer(b'x' * 16, 16)
    assert lib.fc_tangent_lin_describe(100, 64, 64, 0, 1, small, len(line)) == -2 and small.raw == b'x' * 16       # (untouched)
    assert _describe(lib, 100, 64, 64, 0, 1, size=len(line) + 1) == (0, line)
    # the alignment flag alone moves a launch from the direct kernel to the staged one with scalar loads; M <= 16 stays staged
    assert _describe(lib, 100, 64, 64, 0, 0)[1].startswith('staged split=1 loads=scalar tiles=4 kchunks=2 lds=69632 ')
    assert _describe(lib, 100, 64, 16, 0, 1)[1].startswith('staged split=0 loads=vector tiles=1 kchunks=2 lds=17408 ')
    assert pc.parse_route(line) == {'kernel': 'direct', 'grid': 7, 'blocks': 7, 'trips': 1, 'cus': 256}
