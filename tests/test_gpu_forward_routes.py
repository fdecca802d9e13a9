"""One forward launch on every route the host layer can take (csrc/fc_forward_route.hpp): dense rows, the edge split, one round of the
frequency-major kernels, the ring-major kernels with spread half tiles / a last round of half tiles / whole tiles only, the aliased
half-chunk LDS plan, and the frequency-major half tiles of fp32 mode.  Each case first reads from fc_describe_kernels that it is on the
route it is named for, then checks y against the complex128 oracle and the fused epilogue against the separate operators."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import rel_err
from oracle import fieldconv_oracle as orc

import fieldconv_amd
from fieldconv_amd import _env, _lib

pytestmark = pytest.mark.gpu

REDUCED = os.environ.get('FC_MFMA') == 'f16'
TOL = 5e-3 if REDUCED else 1e-5          # tests/test_gpu_parity.py's gate and its FC_MFMA convention

# name -> (N, k, I, O, R, B, arithmetic mode or None, dense rows, the words and fields of the route's description)
CASES = {
    'dense-rows': (300, 8, 8, 8, 4, 1, None, True, ('fc_forward_kernel<dense rows', dict(grid=19, whole=19, half=0, spread=0))),
    'edge-split': (200, 96, 8, 8, 4, 1, None, False, ('(frequency-major', dict(half=0, spread=0, parts=lambda p: p in (2, 4, 8)))),
    'one-round': (3000, 8, 8, 8, 4, 1, None, False, ('(frequency-major', dict(grid=188, whole=188, half=0, spread=0, parts=1))),
    'ring-spread': (4112, 8, 8, 8, 4, 1, None, False, ('(ring-major', dict(grid=512, whole=2, half=510, spread=1))),
    'ring-half-tiles': (8203, 8, 8, 8, 4, 1, None, False, ('(ring-major', dict(grid=512, whole=512, half=2, spread=0))),
    'ring-whole-tiles': (12300, 8, 8, 8, 4, 1, None, False, ('(ring-major', dict(grid=512, whole=769, half=0, spread=0))),
    'ring-aliased-half-chunks': (4112, 8, 64, 64, 6, 3, None, False, ('half-size record chunks, partials aliased onto the slab', dict(grid=512, spread=1))),
    'f32-half-tiles': (4112, 8, 8, 8, 4, 1, 'f32', False, ('(frequency-major', dict(grid=256, whole=256, half=2, spread=0, parts=1))),
}
FIELDS = re.compile(r' grid=(\d+) whole=(\d+) half=(\d+) spread=([01]) lds=(\d+) cus=(\d+)')
H = lambda t: t.detach().cpu().numpy()


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def _route(graph, I, O, B, kind):
    from fieldconv_amd.functional import make_dims
    buf = ctypes.create_string_buffer(1536)
    d = make_dims(graph, I, O, B)
    assert _lib.load().fc_describe_kernels(ctypes.byref(d), kind, buf, len(buf)) == 0
    fwd = buf.value.decode().split(';')[0]
    m = FIELDS.search(fwd)
    assert m, fwd
    got = dict(grid=int(m.group(1)), whole=int(m.group(2)), half=int(m.group(3)), spread=int(m.group(4)))
    parts = re.search(r'parts=(\d+)\)', fwd)
    if parts:
        got['parts'] = int(parts.group(1))
    return fwd, got, int(m.group(6))


@pytest.mark.parametrize('name', sorted(CASES))
def test_forward_on_every_route_vs_oracle_and_fused_epilogue(name, dev):
    if os.environ.get('FC_MFMA') not in (None, '', 'split'):
        pytest.skip('the routes named here are the default mode\'s (the fp32 one is entered with arithmetic())')
    switches = [k for k in _env.SWITCHES if k != 'FC_MFMA' and os.environ.get(k) not in (None, '')]
    if switches:
        pytest.skip('switches set (%s): they move the routes' % ', '.join(switches))
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.functional import _records, field_conv, field_conv_act, field_conv_params, tangent_nonlin
    from fieldconv_amd.graph import SupportGraph
    from fieldconv_amd.nn import FieldConv
    from oracle.torch_composites import FCPrecomp           # the tests build their stencils on the CPU
    N, k, I, O, R, B, mode, dense, (words, fields) = CASES[name]
    data = sphere_support(N, k, seed=4)
    data.epsilon = float(data.logMag.max()) * 1.0001          # use every ring
    edges, sten, _, _ = FCPrecomp(B, R, data.epsilon)(data)
    F = 2 * B + 1
    g = torch.Generator().manual_seed(N + I)
    x = torch.complex(torch.randn(N, I, generator=g), torch.randn(N, I, generator=g))
    x[torch.rand(N, I, generator=g) < 0.02] = 0
    W = torch.complex(torch.randn(O, I, R, F, generator=g), torch.randn(O, I, R, F, generator=g)) * (1.0 / (I * R) ** 0.5)
    addend = torch.complex(torch.randn(N, O, generator=g), torch.randn(N, O, generator=g)).to(dev)
    graph = SupportGraph(edges.to(dev), sten.to(dev), N, allow_factored=not dense)
    with (fieldconv_amd.arithmetic(mode) if mode else contextlib.nullcontext()):
        kind = _records(graph)[0]
        assert (kind == 0) == dense
        fwd, got, cus = _route(graph, I, O, B, kind)
        if cus != 256:
            pytest.skip('the description says cus=%d: the routes are named for the MI355X\'s 256 CUs' % cus)
        assert words in fwd, fwd
        for f, want in fields.items():
            assert want(got.get(f)) if callable(want) else got.get(f) == want, (f, fwd)
        assert got['whole'] + got['half'] // 2 == ((N + 15) // 16) * got.get('parts', 1), fwd          # every tile is dealt once
        y = field_conv(x.to(dev), W.to(dev), graph)
        torch.manual_seed(N)
        conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=1).to(dev)
        bias = torch.empty(1, O).uniform_(-0.4, 0.1, generator=g).to(dev)
        xd = x.to(dev)
        fused = field_conv_act(xd, conv.zonal, conv.spherical, conv.phase, conv.ftype, B, graph, bias, addend=addend)
        separate = tangent_nonlin(field_conv_params(xd, conv.zonal, conv.spherical, conv.phase, conv.ftype, B, graph) + addend, bias)
    y_ref = orc.fieldconv_forward(x.numpy(), edges.numpy(), sten.numpy(), W.numpy())
    err = rel_err(H(y), y_ref)
    print(f'{name}: {fwd}\n  y vs oracle {err:.2e}')
    assert np.all(np.isfinite(H(y))) and err < TOL
    # the in-kernel epilogue (the parts' sum on the edge split): the same arithmetic as the separate operators, bit for bit
    assert torch.equal(fused, separate)
