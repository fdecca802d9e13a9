"""Guard-band canaries over the C ABI (race detection / sanitizers -- GPU ASan and XNACK are not available on this pool,
hence plain canaries).

Every buffer the host layer hands to libfieldconv_hip.so -- outputs, packed filter images, workspaces, saved buffers, gradient
buffers -- is allocated at exactly the size the library's `*_bytes` / `*_floats` queries return.  Here those allocations are
carved out of larger ones whose margins hold a byte pattern; after a forward + backward pass of each entry-point family the margins
must be untouched: a kernel that writes one element past `[0, *_bytes)` of ANY buffer fails the test.  The record arrays are the one
place where the kernels deliberately READ past the last record (reference-side: transforms/fc_precomp.py pads them); the second
test puts NaNs right behind the documented padding and requires bit-identical, finite results."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GUARD = 4096
PATTERN = 0xA5


class GuardedTorch:
    """Stands in for the `torch` module inside fieldconv_amd's host layer: `empty` / `empty_like` on the GPU return views into
    allocations with GUARD bytes of PATTERN on both sides (and the payload pre-filled with the pattern too)."""

    def __init__(self):
        self.blocks = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def _guarded(self, shape, dtype, device):
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = int(np.prod(shape)) if len(shape) else 1
        item = torch.empty((), dtype=dtype).element_size()
        nbytes = n * item
        buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=device)
        self.blocks.append((buf, nbytes))
        if nbytes == 0:
            return torch.empty(shape, dtype=dtype, device=device)
        return buf[GUARD:GUARD + nbytes].view(dtype).view(shape)

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        dev = torch.device(device) if device is not None else torch.device('cpu')
        if dev.type != 'cuda' or kw:
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._guarded(size, dtype or torch.float32, dev)

    def empty_like(self, t, **kw):
        if t.device.type != 'cuda' or kw or not t.is_contiguous():
            return torch.empty_like(t, **kw)
        return self._guarded(tuple(t.shape), t.dtype, t.device)

    def check(self, what):
        torch.cuda.synchronize()
        bad = []
        for idx, (buf, nbytes) in enumerate(self.blocks):
            lo, hi = buf[:GUARD], buf[GUARD + nbytes:]
            if not bool((lo == PATTERN).all()) or not bool((hi == PATTERN).all()):
                first = int((hi != PATTERN).nonzero()[0]) if not bool((hi == PATTERN).all()) else -int((lo != PATTERN).nonzero()[-1]) - 1
                bad.append((idx, nbytes, first))
        assert not bad, f'{what}: writes outside a buffer (allocation index, payload bytes, first offending byte past the end / before the start): {bad[:5]}'
        n = len(self.blocks)
        self.blocks = []
        return n


@pytest.fixture()
def guarded(monkeypatch):
    import fieldconv_amd._launch as launch
    import fieldconv_amd.blocks as blocks
    import fieldconv_amd.functional as Fn
    import fieldconv_amd.graph as graph
    import fieldconv_amd.head as head
    import fieldconv_amd.losses as losses
    import fieldconv_amd.matching as matching
    import fieldconv_amd.norm as norm
    import fieldconv_amd.pooling as pooling
    import fieldconv_amd.transforms.fc_precomp as pre
    import fieldconv_amd.transforms.support_graph as support
    g = GuardedTorch()
    for mod in (launch, Fn, blocks, graph, pre, norm, pooling, losses, head, matching, support):
        monkeypatch.setattr(mod, 'torch', g)
    # the host-side nodes in Python: the C++ nodes allocate inside torch's C++ API, where this stand-in does not reach
    monkeypatch.setenv('FIELDCONV_CPP_NODES', '0')
    return g


def _mesh(N, k, B, R, dev, seed=0):
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.transforms import FCPrecomp
    data = sphere_support(N, k=k, seed=seed, support='p95').to(dev)
    pre = FCPrecomp(B, R, data.epsilon)
    edges, sten, ln, wxp = pre(data)
    return data, edges, sten, ln, wxp


def _cplx(shape, gen, dev):
    return torch.complex(torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)).to(dev)


# configs 2, 3 and 5 at their channel counts / band limits (config 2 at its size: the H-streaming backward), and three ragged shapes
SHAPES = [
    pytest.param(20000, 32, 48, 48, 2, 6, id='config2'),
    pytest.param(1024, 128, 48, 48, 2, 6, id='config3'),
    pytest.param(4999, 24, 64, 64, 3, 6, id='config5'),
    pytest.param(8203, 9, 16, 32, 1, 4, id='ragged-stream-sized'),
    pytest.param(777, 11, 5, 7, 2, 3, id='ragged-small'),
    pytest.param(3001, 7, 40, 24, 3, 5, id='ragged-mid'),
]


@pytest.mark.parametrize('N,k,I,O,B,R', SHAPES)
def test_no_write_outside_any_buffer_fieldconv(guarded, N, k, I, O, B, R):
    """FCPrecomp + graph build, filter packing, forward (geometric records, factored records, dense rows), the whole backward pass with
    parameter gradients and with an explicit filter, TangentLin, TangentNonLin."""
    from fieldconv_amd import functional as Fn
    from fieldconv_amd.graph import SupportGraph, get_graph
    from fieldconv_amd.nn import FieldConv
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(N)
    data, edges, sten, ln, wxp = _mesh(N, k, B, R, dev)
    n = guarded.check('FCPrecomp + graph build')
    x = _cplx((N, I), gen, dev).requires_grad_(True)
    gy = _cplx((N, O), gen, dev)
    for ftype in (0, 1, 2):
        conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=ftype).to(dev)
        y = conv(x, edges, sten)
        torch.autograd.grad(y, [x] + list(conv.parameters()), grad_outputs=gy)
        n += guarded.check(f'FieldConv ftype {ftype} (records)')
    # explicit filter; dense rows and 64-byte factored records as well
    W = (_cplx((O, I, R, 2 * B + 1), gen, dev) * 0.1).requires_grad_(True)
    dense = sten.materialize() if hasattr(sten, 'materialize') else sten
    graphs = {'records': get_graph(edges, sten, N)}
    if N <= 5000:
        graphs['dense rows'] = SupportGraph(edges, dense, N, allow_factored=False)
    for name, g in graphs.items():
        y = Fn.field_conv(x, W, g)
        torch.autograd.grad(y, [x, W], grad_outputs=gy)
        n += guarded.check(f'field_conv explicit filter ({name})')
    re_w, im_w = torch.randn(O, I, device=dev, requires_grad=True), torch.randn(O, I, device=dev, requires_grad=True)
    y = Fn.tangent_lin(x, re_w, im_w)
    torch.autograd.grad(y, [x, re_w, im_w], grad_outputs=gy)
    bias = torch.randn(I, device=dev, requires_grad=True)
    y = Fn.tangent_nonlin(x, bias)
    torch.autograd.grad(y, [x, bias], grad_outputs=_cplx((N, I), gen, dev))
    n += guarded.check('TangentLin / TangentNonLin')
    assert n > 20


@pytest.mark.parametrize('N,k,C,B,R', [pytest.param(1024, 128, 48, 2, 6, id='config3'), pytest.param(4999, 24, 64, 3, 6, id='config5'),
                                       pytest.param(2050, 10, 24, 1, 4, id='ragged')])
def test_no_write_outside_any_buffer_blocks(guarded, N, k, C, B, R):
    """FCResNetBlock, ECHOBlock (descriptor splat + native head) and LiftBlock through the block-level entry points (saved buffers and
    workspaces carved by the library from caller-owned allocations of exactly the queried size)."""
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(N + 1)
    data, edges, sten, ln, wxp = _mesh(N, k, B, R, dev, seed=1)
    guarded.check('FCPrecomp + graph build')
    x = _cplx((N, C), gen, dev).requires_grad_(True)
    blk = FCResNetBlock(C, C, band_limit=B, n_rings=R, ftype=1).to(dev)
    y = blk(x, edges, sten)
    torch.autograd.grad(y, [x] + list(blk.parameters()), grad_outputs=_cplx(tuple(y.shape), gen, dev))
    n = guarded.check('FCResNetBlock')
    echo = ECHOBlock(C, 8, band_limit=B, n_rings=R, ftype=1).to(dev)
    d = echo(x, edges, sten, ln, wxp)
    torch.autograd.grad(d, [x] + list(echo.parameters()), grad_outputs=torch.randn(d.shape, generator=gen).to(dev), allow_unused=True)
    n += guarded.check('ECHOBlock')
    lift = LiftBlock(3, C, n_rings=R, ftype=1).to(dev)
    pos = torch.randn(N, 3, generator=gen).to(dev).requires_grad_(True)
    z = lift(pos, edges, sten[..., B:B + 2])
    torch.autograd.grad(z, [pos] + list(lift.parameters()), grad_outputs=_cplx(tuple(z.shape), gen, dev), allow_unused=True)
    n += guarded.check('LiftBlock')
    assert n > 10


def _close(what, got, want, tol=1e-4):
    """float32 results against the families' float64 restatements.  The sums here have at most 131 terms, so rounding stays below
    131 x 2^-24 = 8e-6 of the largest entry; 1e-4 leaves room for exp / log / sqrt.  A piece that overlaps another is wrong by O(1)."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    scale = max(float(np.max(np.abs(want))), 1e-30)
    err = float(np.max(np.abs(got - want))) / scale
    assert err < tol, (what, err)


def test_no_write_outside_and_no_overlap_inside_family_workspaces(guarded):
    """TangentNorm, mesh pooling, the pair losses, the fused classification head, descriptor matching and the radius search, forward
    and backward, at the smallest shapes that use every piece of their workspaces (an empty mesh, weights and gain; parts = 2, so that
    the two-piece branches run; k = 3 for the two-array top-k; an epsilon that overfills rows).  Writes past a buffer trip the guard
    bands; pieces that overlap INSIDE a workspace show as wrong values against the references the families' own tests use."""
    import _head_ref as href
    import _losses_ref as lref
    import _matching_ref as mref
    import _norm_ref as nref
    from test_gpu_mesh_batch import pool_ref
    from test_gpu_support_graph import radius_ref
    from fieldconv_amd.head import linear_cross_entropy, linear_topk
    from fieldconv_amd.losses import label_smoothing_loss, twin_loss
    from fieldconv_amd.matching import match_descriptors
    from fieldconv_amd.norm import tangent_norm
    from fieldconv_amd.pooling import mesh_pool
    from fieldconv_amd.transforms.support_graph import radius_edges
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(11)

    def D(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)

    # TangentNorm and pooling: (131, 5) complex64, an empty mesh first
    ptr = [0, 0, 70, 131]
    x, gy = nref.features(131, 5, 1).astype(np.complex64), nref.features(131, 5, 2).astype(np.complex64)
    w, gain = nref.weights(131, 3).astype(np.float32), nref.gains(5, 4).astype(np.float32)
    xd, gd = D(x).requires_grad_(True), D(gain).requires_grad_(True)
    y = tangent_norm(xd, gd, D(np.asarray(ptr, dtype=np.int64)), D(w), 1e-5)
    gx, gg = torch.autograd.grad(y, [xd, gd], grad_outputs=D(gy))
    want = (nref.forward(x, ptr, w, gain, 1e-5, np.float64),) + tuple(nref.backward(x, gy, ptr, w, gain, 1e-5, np.float64))
    for name, got, ref in zip(('y', 'gx', 'ggain'), (y, gx, gg), want):
        _close('tangent_norm ' + name, got, np.asarray(ref).reshape(tuple(got.shape)))
    n = guarded.check('tangent_norm')
    g = rng.standard_normal((3, 5)).astype(np.float32)
    for soft_abs, xin in ((True, x), (False, np.ascontiguousarray(x.real))):
        xp = D(xin).requires_grad_(True)
        out = mesh_pool(xp, D(np.asarray(ptr, dtype=np.int64)), 'mean', soft_abs)
        gxp, = torch.autograd.grad(out, [xp], grad_outputs=D(g))
        o_ref, g_ref = pool_ref(xin, ptr, 'mean', soft_abs, g.astype(np.float64))
        _close('mesh_pool out', out, o_ref)
        _close('mesh_pool gx', gxp, g_ref)
    n += guarded.check('mesh_pool')

    # the pair losses
    xS, xT = rng.standard_normal((37, 6)).astype(np.float32), rng.standard_normal((41, 6)).astype(np.float32)
    pp = np.stack((rng.integers(0, 41, 9), rng.integers(0, 37, 9)), 1).astype(np.int64)
    nn = np.stack((rng.integers(0, 41, 11), rng.integers(0, 37, 11)), 1).astype(np.int64)
    yN = rng.random(11).astype(np.float32)
    a, b = D(xS).requires_grad_(True), D(xT).requires_grad_(True)
    loss = twin_loss(a, b, D(pp), D(nn), D(yN), 5.0)
    gS, gT = torch.autograd.grad(loss.sum(), [a, b])
    lp, ln, gS_ref, gT_ref = lref.twin_loss(xS, xT, pp, nn, yN, 5.0)
    _close('twin_loss', loss.reshape(()), lp + ln)
    _close('twin_loss gS', gS, gS_ref)
    _close('twin_loss gT', gT, gT_ref)
    pred, tgt = rng.standard_normal((33, 7)).astype(np.float32), rng.integers(0, 7, 33).astype(np.int64)
    pd_ = D(pred).requires_grad_(True)
    loss = label_smoothing_loss(pd_, D(tgt), 7, 0.1)
    gp, = torch.autograd.grad(loss.sum(), [pd_])
    l_ref, g_ref = lref.label_smoothing(pred, tgt, 7, 0.1)
    _close('label_smoothing', loss.reshape(()), l_ref)
    _close('label_smoothing grad', gp, g_ref)
    n += guarded.check('losses')

    # the fused head with two parts: forward, weight gradient and top-k all take their two-piece layouts
    h, W, bias = (rng.standard_normal(s).astype(np.float32) for s in ((70, 8), (5, 8), (5,)))
    target = rng.integers(0, 5, 70).astype(np.int64)
    hd, Wd, bd = (D(t).requires_grad_(True) for t in (h, W, bias))
    loss = linear_cross_entropy(hd, Wd, bd, D(target), 'mean', 0.1, -100, 2)
    grads = torch.autograd.grad(loss, [hd, Wd, bd])
    want = href.head(h, W, bias, target, 'mean', 0.1, -100)
    for name, got, ref in zip(('loss', 'g_h', 'g_W', 'g_b'), (loss.reshape(()),) + tuple(grads), want):
        _close('linear_cross_entropy ' + name, got, ref)
    idx, zk = linear_topk(D(h), D(W), D(bias), 3, 2)
    z = href.logits(h, W, bias)
    _close('linear_topk values', zk, -np.sort(-z, axis=1)[:, :3])
    _close('linear_topk classes', zk, np.take_along_axis(z, idx.cpu().numpy(), 1))
    n += guarded.check('head')

    # matching with two parts (features as the family's tests draw them), and the radius search with overfull rows
    mS, mT = (0.9 * rng.random((37, 6))).astype(np.float32), (0.9 * rng.random((41, 6))).astype(np.float32)
    idx, d2 = match_descriptors(D(mS), D(mT), k=2, parts=2)
    i_ref, d_ref = mref.topk(mS, mT, 2)
    assert np.array_equal(idx.cpu().numpy(), i_ref)
    _close('match d2', d2, d_ref)
    n += guarded.check('matching')
    pos = rng.random((200, 3)).astype(np.float32)
    edges = radius_edges(D(pos), 0.35, 8).cpu().numpy()
    ref = radius_ref(pos, 0.35, 8)
    assert np.bincount(radius_ref(pos, 0.35, 512)[:, 0], minlength=200).max() > 8         # some rows are overfull
    assert edges.shape == ref.shape and np.array_equal(edges, ref)
    n += guarded.check('radius')
    assert n > 10


@pytest.mark.parametrize('N,k,C,B,R', [pytest.param(20000, 32, 48, 2, 6, id='config2'), pytest.param(1500, 40, 24, 2, 6, id='small')])
def test_record_read_ahead_stays_inside_the_documented_padding(N, k, C, B, R):
    """The kernels stream record chunks past a vertex's (and the array's) last record; FCPrecomp pads the arrays for that
    (transforms/fc_precomp.py: pad_rec, pad_geo).  With the arrays moved to the END of an allocation whose bytes behind the documented
    padding are NaNs instead of zeros, the results must be finite and bit-identical: nothing behind the padding is read into a result."""
    from fieldconv_amd import functional as Fn
    from fieldconv_amd.graph import get_graph
    dev = torch.device('cuda:0')
    gen = torch.Generator().manual_seed(5)
    data, edges, sten, ln, wxp = _mesh(N, k, B, R, dev, seed=2)
    g = get_graph(edges, sten, N)
    assert g.factored
    x = _cplx((N, C), gen, dev).requires_grad_(True)
    gy = _cplx((N, C), gen, dev)
    W = (_cplx((C, C, R, 2 * B + 1), gen, dev) * 0.1).requires_grad_(True)

    def run():
        y = Fn.field_conv(x, W, g)
        gx, gw = torch.autograd.grad(y, [x, W], grad_outputs=gy)
        return y.detach().clone(), gx.clone(), gw.clone()

    ref = run()
    originals = {}
    for name in ('rec_t', 'rec_s', 'geo_t'):
        t = getattr(g, name, None)
        if t is None:
            continue
        originals[name] = t
        tail = 1 << 20
        buf = torch.empty(t.numel() * 4 + tail, dtype=torch.uint8, device=dev)
        buf[t.numel() * 4:].view(torch.float32).fill_(float('nan'))
        moved = buf[:t.numel() * 4].view(torch.float32).view(t.shape)
        moved.copy_(t)
        setattr(g, name, moved)
    g._plans.clear()
    try:
        out = run()
    finally:
        for name, t in originals.items():
            setattr(g, name, t)
        g._plans.clear()
    for a, b in zip(ref, out):
        assert bool(torch.isfinite(torch.view_as_real(b)).all())
        assert torch.equal(a, b)
