"""The pointwise operators -- TangentLin, TangentNonLin (modReLU), softAbs -- on every route of their launchers, against complex128
(inputs, references and expected routes: _pointwise_cases.py, pinned on the CPU by test_pointwise_host.py).

TangentLin (csrc/fc_pointwise.hip) picks between a direct kernel and an LDS-staged one, the latter split or unsplit, with vector
or scalar row loads; which one a launch takes follows N, the channel counts, the operands' alignment and the device's CU count.
Every case here derives N from the device, asserts through fc_tangent_lin_describe that BOTH of its launches take the route it
is named for, and measures y and gx ROW BY ROW on inputs whose rows differ by powers of two inside each 16-row block.  Part two:
rows do not leak into each other -- the kernels load rows beyond the mesh from clamped addresses and zero them afterwards -- so
every row outside a perturbed set is BIT-IDENTICAL whatever the set holds: times 2^40, inf or NaN (values, not faults)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _pointwise_cases as pc
from conftest import rel_err

pytestmark = pytest.mark.gpu
REDUCED = os.environ.get('FC_MFMA') == 'f16'
TOL = 5e-3 if REDUCED else 1e-5          # tests/test_gpu_parity.py's gate and its FC_MFMA convention
TOL_F64 = 1e-12


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def cases(dev):
    return pc.lin_cases(torch.cuda.get_device_properties(dev).multi_processor_count)


def H(t):
    return t.detach().cpu().numpy()


def D(a, dev, offset=0):
    """`a` on the device; offset = 1: as a view one element off the start of its allocation (complex64: 8 bytes off a 16-byte boundary)."""
    a = np.array(a)             # (a writable copy: the generator's arrays are read-only)
    flat = torch.empty(a.size + offset, dtype=torch.from_numpy(a).dtype, device=dev)
    v = flat[offset:].view(a.shape)
    v.copy_(torch.from_numpy(a))
    return v


def require_routes(name, case, xt, gyt, Ret, Imt):
    """Assert from the library's own account, with the real alignment of the tensors, that the forward and the transposed launch of
    this case take the kernels it is named for -- or skip, with the reason, when a development switch has redirected them."""
    from fieldconv_amd import _env, _lib
    lib = _lib.load()
    a_fwd = int(xt.data_ptr() % 16 == 0 and Ret.data_ptr() % 8 == 0 and Imt.data_ptr() % 8 == 0 and case.I % 2 == 0)
    a_bwd = int(gyt.data_ptr() % 16 == 0)
    assert (a_fwd, a_bwd) == ((0, 0) if case.offset else (int(case.I % 2 == 0), 1))
    lines = []
    for K, M, transposed, aligned in ((case.I, case.O, 0, a_fwd), (case.O, case.I, 1, a_bwd)):
        buf = ctypes.create_string_buffer(256)
        assert lib.fc_tangent_lin_describe(case.N, K, M, transposed, aligned, buf, len(buf)) == 0
        lines.append(buf.value.decode())
    missing = {**{'forward ' + k: v for k, v in pc.route_mismatch(pc.parse_route(lines[0]), case.fwd).items()},
               **{'transposed ' + k: v for k, v in pc.route_mismatch(pc.parse_route(lines[1]), case.bwd).items()}}
    switches = {k: v for k, v in _env.active().items() if k != 'FC_MFMA'}         # (the arithmetic mode of the convolutions redirects nothing here)
    if missing and switches:
        pytest.skip('%s: %s not selected under %s: %s' % (name, missing, switches, lines))
    assert not missing, (name, missing, lines)
    print('%s (%d, %d, %d): %s; %s' % ((name, case.N, case.I, case.O) + tuple(lines)))


def run_lin(xt, gyt, Ret, Imt):
    from fieldconv_amd.functional import tangent_lin
    xt = xt.detach().requires_grad_(True)
    y = tangent_lin(xt, Ret, Imt)
    assert type(y.grad_fn).__name__ == '_TangentLinFnBackward'
    gx, gRe, gIm = torch.autograd.grad(y, [xt, Ret, Imt], grad_outputs=gyt)
    return y.detach(), gx, gRe, gIm


def lin_tensors(case, dev):
    x, gy, Re, Im, _ = pc.inputs(case.N, case.I, case.O)
    return (D(x, dev, case.offset), D(gy, dev, case.offset), D(Re, dev).requires_grad_(True), D(Im, dev).requires_grad_(True))


# ------------------------------------------------------------------ 4a: every route of the TangentLin launchers
@pytest.mark.parametrize('name', pc.LIN_NAMES)
def test_tangent_lin_on_every_route(name, cases, dev):
    case = cases[name]
    pc.assert_lin_conditions(case.N, case.I, case.O)            # (conditions on the inputs, at this device's N)
    xt, gyt, Ret, Imt = lin_tensors(case, dev)
    require_routes(name, case, xt, gyt, Ret, Imt)
    y, gx, gRe, gIm = run_lin(xt, gyt, Ret, Imt)
    y_ref, gx_ref, gRe_ref, gIm_ref = pc.lin_reference(case.N, case.I, case.O)
    assert all(np.isfinite(H(t).view(np.float32)).all() for t in (y, gx, gRe, gIm))
    errs = (pc.rowwise_err(H(y), y_ref), pc.rowwise_err(H(gx), gx_ref), rel_err(H(gRe), gRe_ref), rel_err(H(gIm), gIm_ref))
    print('  %s: row-wise y %.2e gx %.2e; global gRe %.2e gIm %.2e' % ((name,) + errs))
    y2, gx2, gRe2, gIm2 = run_lin(xt, gyt, Ret, Imt)
    assert max(errs) < TOL, errs
    assert torch.equal(gRe, gRe2) and torch.equal(gIm, gIm2) and torch.equal(y, y2) and torch.equal(gx, gx2)


def test_tangent_lin_gemm_route_in_double_precision(dev):
    """_TangentLinGemmFn (three fc_cgemm products) called directly on complex128 with float64 weights, 7 -> 70 channels."""
    from fieldconv_amd.functional import _TangentLinGemmFn
    N, I, O = pc.GEMM_F64_CASE
    x, gy, Re, Im, _ = pc.inputs(N, I, O)
    xt = D(x.astype(np.complex128), dev).requires_grad_(True)
    Ret, Imt = D(Re.astype(np.float64), dev).requires_grad_(True), D(Im.astype(np.float64), dev).requires_grad_(True)
    y = _TangentLinGemmFn.apply(xt, Ret, Imt)
    gx, gRe, gIm = torch.autograd.grad(y, [xt, Ret, Imt], grad_outputs=D(gy.astype(np.complex128), dev))
    assert y.dtype == gx.dtype == torch.complex128 and gRe.dtype == torch.float64
    y_ref, gx_ref, gRe_ref, gIm_ref = pc.lin_reference(N, I, O)
    errs = (pc.rowwise_err(H(y), y_ref), pc.rowwise_err(H(gx), gx_ref), rel_err(H(gRe), gRe_ref), rel_err(H(gIm), gIm_ref))
    print('  gemm f64 (%d, %d, %d): row-wise y %.2e gx %.2e; global gRe %.2e gIm %.2e' % ((N, I, O) + errs))
    assert max(errs) < TOL_F64, errs


# ------------------------------------------------------------------ 4b: containment
@pytest.mark.parametrize('name', pc.CONTAINMENT_NAMES)
def test_tangent_lin_rows_do_not_leak_into_each_other(name, cases, dev):
    case = cases[name]
    xt, gyt, Ret, Imt = lin_tensors(case, dev)
    require_routes(name, case, xt, gyt, Ret, Imt)
    x, gy = pc.inputs(case.N, case.I, case.O)[:2]
    P = pc.perturbed_rows(case.N)
    others = np.ones(case.N, bool)
    others[P] = False
    assert P.size >= 2 and P[-1] == case.N - 1 and others.sum() >= case.N - P.size
    clean = [H(t) for t in run_lin(xt, gyt, Ret, Imt)[:2]]
    assert np.isfinite(clean[0].view(np.float32)).all() and np.isfinite(clean[1].view(np.float32)).all()
    for label, value in (('2^40', None), ('inf', np.inf), ('nan', np.nan)):
        for which, base in ((0, x), (1, gy)):               # x[P] -> y, then gy[P] -> gx
            pert = base.copy()
            pert[P] = pert[P] * np.float32(2.0 ** pc.PERTURB_EXP) if value is None else np.complex64(complex(value, value))
            pt = D(pert, dev, case.offset)
            got = H(run_lin(pt if which == 0 else xt, pt if which == 1 else gyt, Ret, Imt)[which])
            what = ('y', 'gx')[which]
            assert np.isfinite(got[others].view(np.float32)).all(), (what, label)
            assert np.array_equal(got[others], clean[which][others]), ('%s rows outside the perturbed set changed' % what, label)
            if value is not None:
                assert not np.isfinite(got[P].view(np.float32)).all(), (what, label)         # (the perturbation did arrive)


# ------------------------------------------------------------------ 4c: TangentNonLin and softAbs, fp32
@pytest.mark.parametrize('N,C', pc.NONLIN_SHAPES)
def test_tangent_nonlin_and_soft_abs_rowwise(N, C, dev):
    from fieldconv_amd.functional import soft_abs, tangent_nonlin
    pc.assert_nonlin_conditions(N, C)
    x, gy, _, _, bias = pc.inputs(N, C, C)
    xt, gyt, bt = D(x, dev).requires_grad_(True), D(gy, dev), D(bias, dev).requires_grad_(True)
    y = tangent_nonlin(xt, bt)
    assert type(y.grad_fn).__name__ == '_TangentNonLinFnBackward'
    gx, gb = torch.autograd.grad(y, [xt, bt], grad_outputs=gyt)
    y_ref, gx_ref, gb_ref = pc.nonlin_reference(N, C)
    errs = [pc.rowwise_err(H(y), y_ref), pc.rowwise_err(H(gx), gx_ref), rel_err(H(gb).reshape(-1), gb_ref.reshape(-1))]
    box = pc.origin_box(x)
    assert box.any() or N * C < 4
    assert np.array_equal(H(y)[box], x[box]) and np.array_equal(H(gx)[box], gy[box])          # pass through bit-exactly; gx = gy there
    gx2, gb2 = torch.autograd.grad(tangent_nonlin(xt, bt), [xt, bt], grad_outputs=gyt)
    assert torch.equal(gb, gb2) and torch.equal(gx, gx2)
    # softAbs and its VJP on the same x, cotangent Re gy
    sy = soft_abs(xt)
    assert type(sy.grad_fn).__name__ == '_SoftAbsFnBackward' and sy.dtype == torch.float32
    sgx, = torch.autograd.grad(sy, [xt], grad_outputs=gyt.real.contiguous())
    sy_ref, sgx_ref = pc.soft_abs_reference(N, C)
    errs += [pc.rowwise_err(H(sy), sy_ref), pc.rowwise_err(H(sgx), sgx_ref)]
    assert not H(sy)[box].any() and not H(sgx)[box].any()
    print('  (%d, %d): row-wise y %.2e gx %.2e; gbias %.2e; softAbs row-wise %.2e / %.2e' % ((N, C) + tuple(errs)))
    assert max(errs) < TOL, errs


# ------------------------------------------------------------------ 4d: TangentNonLin in double precision
@pytest.mark.parametrize('N,C', pc.NONLIN_F64_SHAPES)
def test_tangent_nonlin_f64_against_longdouble(N, C, dev):
    from fieldconv_amd.functional import tangent_nonlin
    pc.assert_nonlin_conditions(N, C)
    x, gy, _, _, bias = pc.inputs(N, C, C)
    xt = D(x.astype(np.complex128), dev).requires_grad_(True)
    bt = D(bias.astype(np.float64), dev).requires_grad_(True)
    y = tangent_nonlin(xt, bt)
    assert type(y.grad_fn).__name__ == '_TangentNonLinF64FnBackward' and y.dtype == torch.complex128
    gx, gb = torch.autograd.grad(y, [xt, bt], grad_outputs=D(gy.astype(np.complex128), dev))
    (yr, yi), (gr, gi), gb_ref = pc.nonlin_reference_longdouble(N, C)
    L = np.longdouble
    parts = lambda t: np.stack([H(t).real.astype(L), H(t).imag.astype(L)], axis=-1)
    errs = (pc.rowwise_err(parts(y), np.stack([yr, yi], axis=-1)), pc.rowwise_err(parts(gx), np.stack([gr, gi], axis=-1)),
            rel_err(H(gb).astype(L).reshape(-1), gb_ref.reshape(-1)))
    box = pc.origin_box(x)
    assert np.array_equal(H(y)[box], x[box].astype(np.complex128)) and np.array_equal(H(gx)[box], gy[box].astype(np.complex128))
    print('  f64 (%d, %d): row-wise y %.2e gx %.2e; gbias %.2e' % ((N, C) + errs))
    assert max(errs) < TOL_F64, errs
