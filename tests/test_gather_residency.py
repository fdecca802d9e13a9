"""The gather kernel of the H-streaming backward with its work item decoupled from the 16-vertex tile (fc_backward_stream.hpp: groups of
WPG consecutive vertices, record address from the vertex, plan_gather).

Shapes: the smallest at which the arrangement is selected and the grouping can go wrong -- 3 072 vertices (the streaming threshold: 192
tiles), 3 075 (no multiple of the group nor of the tile: the last tile holds three vertices, its last group with a vertex has three of
four, three more groups of it have none and still owe the records their zero rows), 8 203 (ragged last tile, more work items than
places in the grid: several rounds) at the default layer, and one two-walk layer (64 channels, band limit 3: the k range in two halves).
One vertex of every mesh has no out-edges and another no in-edges.

Each case: gx and the three parameter gradients (and y) against the fp32 data / filter kernel pair of the same process at the suite's
1e-5 gate, two runs bit for bit, and guard bands around every buffer the host layer hands to the library -- the H workspace among them."""
import ctypes
import os

import pytest
import torch

from conftest import rel_err
from test_gpu_canary import GuardedTorch

pytestmark = pytest.mark.gpu


@pytest.fixture()
def guarded(monkeypatch):
    import fieldconv_amd._launch as launch
    import fieldconv_amd.blocks as blocks
    import fieldconv_amd.functional as Fn
    import fieldconv_amd.graph as graph
    import fieldconv_amd.transforms.fc_precomp as pre
    g = GuardedTorch()
    for mod in (launch, Fn, blocks, graph, pre):
        monkeypatch.setattr(mod, 'torch', g)
    monkeypatch.setenv('FIELDCONV_CPP_NODES', '0')      # (the C++ nodes allocate inside torch's C++ API, where the stand-in does not reach)
    return g


def _mesh_with_isolated_vertices(N, k, B, R, dev, no_out, no_in):
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.transforms import FCPrecomp
    data = sphere_support(N, k=k, seed=N + k, support='p95')
    keep = (data.supp_edges[:, 0] != no_out) & (data.supp_edges[:, 1] != no_in)
    for name in ('supp_edges', 'logMag', 'logAng', 'xp'):
        setattr(data, name, getattr(data, name)[keep].contiguous())
    data = data.to(dev)
    edges, sten = FCPrecomp(B, R, data.epsilon)(data)[:2]
    for col in (0, 1):      # whichever column the backward walks, one vertex has no edge in it
        assert int(torch.bincount(edges[:, col], minlength=N).min()) == 0
    return edges, sten


@pytest.mark.parametrize('N,k,C,B,R', [
    pytest.param(3072, 16, 48, 2, 6, id='threshold-3072'),
    pytest.param(3075, 24, 48, 2, 6, id='ragged-group-3075'),
    pytest.param(8203, 32, 48, 2, 6, id='several-rounds-8203'),
    pytest.param(3075, 16, 64, 3, 6, id='two-walks-halves-3075'),
])
def test_gather_groups_against_the_fp32_kernel_pair(guarded, N, k, C, B, R):
    if os.environ.get('FC_MFMA') not in (None, '', 'split') or os.environ.get('FC_BWD_STREAM') not in (None, ''):
        pytest.skip('the arrangement exists in the default arithmetic mode only')
    import fieldconv_amd
    from fieldconv_amd import _lib
    from fieldconv_amd.nn import FieldConv
    dev = torch.device('cuda:0')
    # a vertex of the last (ragged) group without out-edges, one in the middle of a tile without in-edges
    edges, sten = _mesh_with_isolated_vertices(N, k, B, R, dev, no_out=N - 2, no_in=37)
    lib = _lib.load()
    dims = _lib.FcDims(N, int(edges.shape[0]), C, C, R, B)
    assert lib.fc_backward_streams(ctypes.byref(dims), 1)
    buf = ctypes.create_string_buffer(1024)
    assert lib.fc_describe_kernels(ctypes.byref(dims), 2, buf, len(buf)) == 0
    assert b'fc_backward_gather_kernel' in buf.value and b'wavefronts,' in buf.value, buf.value
    print(buf.value.decode().split(';')[0])

    conv = FieldConv(C, C, band_limit=B, n_rings=R, ftype=1).to(dev)
    gen = torch.Generator().manual_seed(N)
    x = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
    gy = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev)

    def step():
        y = conv(x, edges, sten)
        return (y.detach(),) + torch.autograd.grad(y, [x] + list(conv.parameters()), grad_outputs=gy)

    got = step()
    again = step()
    assert guarded.check('two passes of the streaming arrangement') > 0
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    with fieldconv_amd.arithmetic('f32'):
        ref = step()
    errs = [rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) for a, b in zip(got, ref)]
    print('y, gx, g_zonal, g_spherical, g_phase against the fp32 kernel pair:', ['%.1e' % e for e in errs])
    assert len(errs) == 5 and all(e == e for e in errs) and max(errs) < 1e-5, errs
