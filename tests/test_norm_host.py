"""Host-side checks of TangentNorm (fieldconv_amd.norm, csrc/fc_norm.hip): the numpy restatement's gradients against central
differences of the restatement itself, the C ABI surface, the public names, the module's state and argument validation
(everything is rejected before a device is needed).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _norm_ref as nref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {'fc_tangent_norm_workspace_bytes', 'fc_tangent_norm_forward', 'fc_tangent_norm_backward'}


@pytest.mark.parametrize('weighted', [False, True])
def test_restated_gradients_equal_central_differences(weighted):
    N, C, ptr, eps = 7, 3, [0, 3, 7], 1e-3
    x, gy = nref.features(N, C, 1), nref.features(N, C, 2)
    w, gain = (nref.weights(N, 3) if weighted else None), nref.gains(C, 4)
    gx, ggain = nref.backward(x, gy, ptr, w, gain, eps, np.float64)
    h = 1e-5
    num_x = np.zeros_like(x)
    for n in range(N):
        for c in range(C):
            for part in (1.0, 1j):
                d = np.zeros_like(x)
                d[n, c] = h * part
                num_x[n, c] += part * (nref.loss(x + d, gy, ptr, w, gain, eps) - nref.loss(x - d, gy, ptr, w, gain, eps)) / (2 * h)
    num_g = np.zeros(C)
    for c in range(C):
        d = np.zeros(C)
        d[c] = h
        num_g[c] = (nref.loss(x, gy, ptr, w, gain + d, eps) - nref.loss(x, gy, ptr, w, gain - d, eps)) / (2 * h)
    # central differences of a smooth function at h = 1e-5: truncation ~ h^2 = 1e-10, rounding ~ 1e-15 / h = 1e-10
    assert np.abs(gx - num_x).max() <= 1e-8 * np.abs(gx).max()
    assert np.abs(ggain - num_g).max() <= 1e-8 * np.abs(ggain).max()


def test_restatement_normalises_every_mesh_and_channel():
    ptr = list(nref.STANDARD_PTR)
    x, w = nref.features(ptr[-1], 5, 5), nref.weights(ptr[-1], 6)
    y = nref.forward(x, ptr, w, None, 0.0, np.float64)
    for b in range(1, len(ptr) - 1):
        p0, p1 = ptr[b], ptr[b + 1]
        ms = (w[p0:p1, None] * np.abs(y[p0:p1]) ** 2).sum(0) / w[p0:p1].sum()
        assert np.abs(ms - 1).max() <= 1e-12
    y32 = nref.forward(x, ptr, w, None, 0.0, np.float32)
    assert y32.dtype == np.complex64 and 0 < np.abs(y32 - y).max() <= 1e-5 * np.abs(y).max()
    # a mesh without mass: r = 1 / sqrt(eps); the gradient has no second term
    w0 = w.copy()
    w0[64:129] = 0
    y0 = nref.forward(x, ptr, w0, None, 1e-2, np.float64)
    assert np.abs(y0[64:129] - 10 * x[64:129]).max() <= 1e-12 * np.abs(y0).max()
    gy = nref.features(ptr[-1], 5, 7)
    gx0, _ = nref.backward(x, gy, ptr, w0, None, 1e-2, np.float64)
    assert np.abs(gx0[64:129] - 10 * gy[64:129]).max() <= 1e-12 * np.abs(gx0).max()


def test_header_binding_and_library_export_the_new_symbols():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES)
    assert 'fc_norm.hip' in build.SOURCES and 'fc_segment.hpp' in build.HEADERS
    assert [len(_lib.SIGNATURES[n][1]) for n in sorted(SYMBOLS)] == [15, 14, 4]
    lib = ctypes.CDLL(build.build_native())
    assert all(hasattr(lib, n) for n in SYMBOLS) and _lib.load().fc_abi_version() == 11


def test_limits_are_those_of_the_pooling_section():
    from fieldconv_amd import _lib
    lib = _lib.load()
    assert lib.fc_tangent_norm_workspace_bytes(386, 5, 48, 0) > 0
    assert lib.fc_tangent_norm_workspace_bytes(386, 5, 48, 1) >= lib.fc_tangent_norm_workspace_bytes(386, 5, 48, 0)
    for N, B, C, dt in ((386, 0, 48, 0), (386, 5, 0, 0), (386, 5, 64 * 65535 + 1, 0), (-1, 5, 48, 0), (386, 5, 48, 2), (2 ** 31 - 65, 1, 1, 0)):
        assert lib.fc_tangent_norm_workspace_bytes(N, B, C, dt) == 0
        # bad dims are refused before any pointer is looked at or anything is launched
        assert lib.fc_tangent_norm_forward(None, None, None, None, N, B, C, dt, 1e-5, None, None, None, 0, None) == -1
        assert lib.fc_tangent_norm_backward(None, None, None, None, None, None, N, B, C, dt, None, None, None, 0, None) == -1
    assert lib.fc_tangent_norm_forward(None, None, None, None, 386, 5, 48, 0, -1.0, None, None, None, 0, None) == -1


def test_public_names():
    from fieldconv_amd import functional, nn, norm
    assert functional.tangent_norm is norm.tangent_norm
    assert 'TangentNorm' in nn.__all__ and nn.TangentNorm is not None


def test_module_state():
    from fieldconv_amd.nn import TangentNorm
    m = TangentNorm(5)
    sd = m.state_dict()
    assert list(sd) == ['gain'] and tuple(sd['gain'].shape) == (1, 5) and bool((sd['gain'] == 1).all()) and sd['gain'].dtype == torch.float32
    assert m.gain.requires_grad and len(list(m.parameters())) == 1
    plain = TangentNorm(5, affine=False)
    assert not plain.state_dict() and not list(plain.parameters()) and plain.gain is None
    assert m.double().gain.dtype == torch.float64
    assert 'eps=0.001' in repr(TangentNorm(5, eps=1e-3)) and 'affine=False' in repr(plain)
    for bad in (dict(channels=0), dict(channels=2.5), dict(channels=4, eps=-1.0)):
        with pytest.raises(ValueError):
            TangentNorm(**bad)


@pytest.mark.parametrize('change', ['x 1-d', 'x 3-d', 'no channels', 'gain dtype', 'gain length', 'gain shape', 'w dtype', 'w length', 'w shape',
                                    'eps negative', 'eps nan', 'ptr dtype', 'ptr end', 'ptr descending', 'ptr 2-d', 'x not a tensor'])
def test_bad_arguments_raise_value_error(change):
    from fieldconv_amd.norm import tangent_norm
    x = torch.zeros(6, 4, dtype=torch.complex64)
    kw = dict(gain=torch.ones(1, 4), ptr=torch.tensor([0, 2, 6]), w=torch.ones(6, 1), eps=1e-5)
    if change == 'x 1-d':
        x = x[:, 0]
    elif change == 'x 3-d':
        x = x[None]
    elif change == 'no channels':
        x, kw['gain'] = x[:, :0], None
    elif change == 'gain dtype':
        kw['gain'] = torch.ones(1, 4, dtype=torch.float64)
    elif change == 'gain length':
        kw['gain'] = torch.ones(1, 5)
    elif change == 'gain shape':
        kw['gain'] = torch.ones(4, 1)
    elif change == 'w dtype':
        kw['w'] = torch.ones(6, dtype=torch.float64)
    elif change == 'w length':
        kw['w'] = torch.ones(5)
    elif change == 'w shape':
        kw['w'] = torch.ones(1, 6)
    elif change == 'eps negative':
        kw['eps'] = -1e-5
    elif change == 'eps nan':
        kw['eps'] = float('nan')
    elif change == 'ptr dtype':
        kw['ptr'] = torch.tensor([0, 2, 6], dtype=torch.int32)
    elif change == 'ptr end':
        kw['ptr'] = torch.tensor([0, 2, 5])
    elif change == 'ptr descending':
        kw['ptr'] = torch.tensor([0, 4, 2, 6])
    elif change == 'ptr 2-d':
        kw['ptr'] = torch.tensor([[0, 6]])
    elif change == 'x not a tensor':
        x = [[1j]]
    with pytest.raises(ValueError):
        tangent_norm(x, **kw)


def test_real_and_half_features_raise_type_error():
    from fieldconv_amd.norm import tangent_norm
    for dtype in (torch.float32, torch.float64, torch.float16, torch.bfloat16):
        with pytest.raises(TypeError):
            tangent_norm(torch.zeros(6, 4, dtype=dtype))


def test_there_is_no_cpu_path():
    from fieldconv_amd.nn import TangentNorm
    from fieldconv_amd.norm import tangent_norm
    x = torch.zeros(6, 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError):
        tangent_norm(x)
    with pytest.raises(RuntimeError):
        tangent_norm(x.to(torch.complex128), torch.ones(1, 4, dtype=torch.float64), torch.tensor([0, 2, 6]), torch.ones(6, dtype=torch.float64))
    with pytest.raises(RuntimeError):
        TangentNorm(4)(x, torch.tensor([0, 6]))
