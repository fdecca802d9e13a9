"""Mini-batches of meshes on the device: MeshBatch through the product path against the reference's accumulated single-mesh
steps (tests/golden/mesh_batch.npz, made by tests/golden/make_golden_batch.py), the union against its single meshes through
our own path, the per-mesh pooling kernels (csrc/fc_segment.hip) against a numpy float64 restatement, and the batched
farthest-point sampling / radius search (csrc/fc_support.hip) against the numpy restatements of tests/test_gpu_support_graph.py
per mesh."""
import math
import os
import sys

import numpy as np
import pytest
import torch

from conftest import load_golden, rel_err
from oracle import fieldconv_oracle as orc

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


class Data:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def H(t):
    return t.detach().cpu().numpy()


# ---------------------------------------------------------------- one batched step = the reference's accumulated steps
def _fixture_batch(dev, labels):
    from fieldconv_amd.data import MeshBatch
    c = load_golden('mesh_batch.npz')
    m = c['meshes']
    meshes = []
    off = 0
    for i, n in enumerate(m['sizes']):
        n = int(n)
        y = m['y_mesh'][i:i + 1] if labels == 'mesh' else m['y_vertex'][off:off + n]
        off += n
        meshes.append(Data(pos=D(m[f'pos_{i}'], dev), sample_idx=torch.arange(n, device=dev), supp_edges=D(m[f'edges_{i}'], dev),
                           logMag=D(m[f'logMag_{i}'], dev), logAng=D(m[f'logAng_{i}'], dev), xp=D(m[f'xp_{i}'], dev),
                           w=D(m[f'w_{i}'], dev), y=D(y, dev)))
    return c, m, MeshBatch.from_list(meshes)


def _check_against_accumulated(c, logits, losses, net):
    """Gates: test_segmentation_net_golden's for the same depth (rel_err < TOL for logits, < 5 TOL for gradients, the loss to
    1e-5), each widened to 4 x the reference's own deviation under a few-ulp perturbation of its input (the fixture's cond_* /
    gcond_<name>), as test_correspondence_net_golden does -- and for no other reason."""
    e_logits = rel_err(H(logits), c['logits'])
    e_loss = float(np.max(np.abs(H(losses) - c['losses']) / np.maximum(1.0, np.abs(c['losses']))))
    loss = losses.mean()          # == sum_b L_b / B, what the accumulated steps differentiate
    params = dict(net.named_parameters())
    assert sum(p.numel() for p in params.values()) == int(c['n_params'])
    grads = torch.autograd.grad(loss, list(params.values()))
    report = sorted(((rel_err(H(g), c['g_' + name]), float(c['gcond_' + name]), name) for (name, _), g in zip(params.items(), grads)),
                    reverse=True)
    print('logits err %.2e (twin %.1e), loss err %.2e (twin %.1e), worst gradient errs %s' % (
        e_logits, float(c['cond_logits']), e_loss, float(c['cond_loss']), ['%s %.1e / twin %.1e' % (n, e, cd) for e, cd, n in report[:5]]))
    assert e_logits < max(TOL, 4 * float(c['cond_logits']))
    assert e_loss < max(1e-5, 4 * float(c['cond_loss']))
    for e, cond, name in report:
        assert e < max(5 * TOL, 4 * cond), (name, e, cond)


def _fill(net):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from param_fill import fill_params
    return fill_params(net)


def test_batched_classification_step_equals_accumulated_reference_steps(dev):
    """classification.ipynb's topology on the union of four meshes (40, 97, 64, 150 vertices), ONE step: our FCPrecomp on the
    batch, the strided lift slice, two FCResNetBlocks, FieldConv, MeshPool + bias, cross-entropy per mesh, mean -- against the
    reference run one mesh at a time with L / 4 accumulated."""
    from fieldconv_amd.nn import FCResNetBlock, FieldConv, LiftBlock, MeshPool
    from fieldconv_amd.transforms import FCPrecomp
    c, m, batch = _fixture_batch(dev, 'mesh')
    B, R, C, K = int(m['B']), int(m['R']), int(m['C']), int(m['n_classes'])
    kw = dict(band_limit=B, n_rings=R, ftype=1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lift = LiftBlock(3, C, n_rings=R, ftype=1)
            self.resnet1 = FCResNetBlock(C, C, **kw)
            self.resnet2 = FCResNetBlock(C, C, **kw)
            self.conv_out = FieldConv(C, K, **kw)
            self.bias = torch.nn.Parameter(torch.zeros(1, K))
            self.pool = MeshPool('mean')

        def forward(self, data, pre):
            edges, sten, _, _ = pre(data)
            x = self.lift(data.pos[data.sample_idx], edges, sten[..., B:B + 2])
            x = self.resnet2(self.resnet1(x, edges, sten), edges, sten)
            return self.pool(self.conv_out(x, edges, sten), data.ptr) + self.bias

    net = _fill(Net()).to(dev)
    pre = FCPrecomp(B, R, float(m['eps']))
    logits = net(batch, pre)
    assert pre(batch)[0].shape[0] == sum(int(m[f'kept_edges_{i}']) for i in range(batch.num_meshes))
    assert logits.shape == (batch.num_meshes, K)
    losses = torch.nn.functional.cross_entropy(logits, batch.y, reduction='none')
    _check_against_accumulated(c['classification'], logits, losses, net)
    # the reference's own float32 rounding, for scale: its float32 run against its float64 run
    print('reference float32 vs float64: logits %.1e' % rel_err(c['classification']['logits'], c['classification']['logits64']))


def test_batched_segmentation_step_equals_accumulated_reference_steps(dev):
    """The segmentation topology (LiftBlock, two FCResNetBlocks, ECHOBlock) with per-vertex labels: the per-mesh loss means through
    mesh_mean, then their mean."""
    from fieldconv_amd.functional import mesh_mean
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock
    from fieldconv_amd.transforms import FCPrecomp
    c, m, batch = _fixture_batch(dev, 'vertex')
    B, R, C, K = int(m['B']), int(m['R']), int(m['C']), int(m['n_classes'])
    kw = dict(band_limit=B, n_rings=R, ftype=1)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.lift = LiftBlock(3, C, n_rings=R, ftype=1)
            self.resnet1 = FCResNetBlock(C, C, **kw)
            self.resnet2 = FCResNetBlock(C, C, **kw)
            self.echo = ECHOBlock(C, K, n_des=int(m['n_des']), n_bins=int(m['n_bins']), **kw)

        def forward(self, data, pre):
            edges, sten, ln, wxp = pre(data)
            x = self.lift(data.pos[data.sample_idx], edges, sten[..., B:B + 2])
            x = self.resnet2(self.resnet1(x, edges, sten), edges, sten)
            return self.echo(x, edges, sten, ln, wxp)

    net = _fill(Net()).to(dev)
    logits = net(batch, FCPrecomp(B, R, float(m['eps'])))
    assert batch.y.shape == (batch.num_nodes,)
    per_vertex = torch.nn.functional.cross_entropy(logits, batch.y, reduction='none')
    losses = mesh_mean(per_vertex[:, None], batch.ptr)[:, 0]
    _check_against_accumulated(c['segmentation'], logits, losses, net)


# ---------------------------------------------------------------- the union against its single meshes, our own path
def _sphere_batch(sizes, k, dev):
    from fieldconv_amd.data import MeshBatch, sphere_support
    meshes = [sphere_support(n, k=k, seed=3 + i, support='p95').to(dev) for i, n in enumerate(sizes)]
    eps = max(m.epsilon for m in meshes)
    return MeshBatch.from_list(meshes), eps


def _cplx(shape, gen, dev):
    return torch.complex(torch.randn(shape, generator=gen), torch.randn(shape, generator=gen)).to(dev)


def test_union_rows_equal_the_single_meshes(dev):
    """A consistency check (the accuracy evidence is above): rows ptr[b]:ptr[b+1] of each module's output on the union against the
    same module on batch.mesh(b).  Not bitwise: the union may take another kernel arrangement."""
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, FieldConv, LiftBlock
    from fieldconv_amd.transforms import FCPrecomp
    B, R, C = 2, 6, 16
    batch, eps = _sphere_batch((300, 777, 257, 512), 12, dev)
    gen = torch.Generator().manual_seed(8)
    ptr = batch.ptr.tolist()
    N = ptr[-1]
    x = _cplx((N, C), gen, dev)
    pos = torch.randn(N, 3, generator=gen).to(dev)
    torch.manual_seed(5)
    kw = dict(band_limit=B, n_rings=R, ftype=1)
    mods = dict(conv=FieldConv(C, C, **kw).to(dev), block=FCResNetBlock(C, C, **kw).to(dev),
                echo=ECHOBlock(C, 8, **kw).to(dev), lift=LiftBlock(3, C, n_rings=R, ftype=1).to(dev))

    def run(data, rows):
        edges, sten, ln, wxp = FCPrecomp(B, R, eps)(data)
        with torch.no_grad():
            return dict(conv=mods['conv'](x[rows], edges, sten), block=mods['block'](x[rows], edges, sten),
                        echo=mods['echo'](x[rows], edges, sten, ln, wxp), lift=mods['lift'](pos[rows], edges, sten[..., B:B + 2]))

    whole = run(batch, slice(0, N))
    worst = {}
    for b in range(batch.num_meshes):
        rows = slice(ptr[b], ptr[b + 1])
        single = run(batch.mesh(b), rows)
        for name in mods:
            worst[name] = max(worst.get(name, 0.0), rel_err(H(whole[name][rows]), H(single[name])))
    print('union vs single meshes:', {k: '%.1e' % v for k, v in worst.items()})
    for name, e in worst.items():
        assert e < TOL, (name, e)


def test_union_of_four_1024_meshes_against_the_oracle(dev):
    """4 x 1 024 vertices: the union is large enough for the arrangements small meshes never reach (the streaming backward pass
    starts at 3 072 vertices).  Forward and gradients against the CPU oracle on the union."""
    from fieldconv_amd import _lib
    from fieldconv_amd.nn import FieldConv
    from fieldconv_amd.transforms import FCPrecomp
    B, R, I, O = 2, 6, 48, 48
    batch, eps = _sphere_batch((1024,) * 4, 16, dev)
    N = batch.num_nodes
    assert N == 4096
    edges, sten, _, _ = FCPrecomp(B, R, eps)(batch)
    lib = _lib.load()
    print('backward streams for the union:', lib.fc_backward_streams(_lib.FcDims(N=N, E=int(edges.shape[0]), I=I, O=O, R=R, B=B), 1))
    gen = torch.Generator().manual_seed(2)
    x = _cplx((N, I), gen, dev).requires_grad_(True)
    gy = _cplx((N, O), gen, dev)
    torch.manual_seed(1)
    conv = FieldConv(I, O, band_limit=B, n_rings=R, ftype=1).to(dev)
    y = conv(x, edges, sten)
    gx, gz, gs, gp = torch.autograd.grad(y, [x, conv.zonal, conv.spherical, conv.phase], grad_outputs=gy)
    z, s, p = (H(t) for t in (conv.zonal, conv.spherical, conv.phase))
    W = orc.effective_filter(z, s, p, 1, B)
    dense = H(sten.materialize() if hasattr(sten, 'materialize') else sten)
    y_ref = orc.fieldconv_forward(H(x), H(edges), dense, W)
    gx_ref, gW_ref = orc.fieldconv_backward(H(x), H(edges), dense, W, H(gy))
    gz_ref = orc.effective_filter_vjp(gW_ref, z, s, p, 1, B)[0]
    errs = dict(y=rel_err(H(y), y_ref), gx=rel_err(H(gx), gx_ref), gzonal=rel_err(H(gz), gz_ref))
    print('union of 4 x 1024 vs oracle:', {k: '%.1e' % v for k, v in errs.items()})
    assert all(v < TOL for v in errs.values()), errs
    # and no edge crosses a mesh boundary
    e = H(edges)
    assert np.array_equal(e[:, 0] // 1024, e[:, 1] // 1024)


# ---------------------------------------------------------------- pooling kernels
def pool_ref(x, ptr, reduce, soft_abs, g=None):
    """float64 restatement: out (B,C) and, with g (B,C), the VJP.  The origin box is tested on the input's own values with the
    threshold in the input's precision (1e-7 rounded to float32 for float32 input), strictly."""
    eps = float(np.float32(1e-7)) if x.dtype in (np.float32, np.complex64) else 1e-7
    xd = x.astype(np.complex128 if soft_abs else np.float64)
    if soft_abs:
        org = (np.abs(xd.real) < eps) & (np.abs(xd.imag) < eps)
        v = np.where(org, 0.0, np.abs(xd))
    else:
        v = xd
    Bn, C = len(ptr) - 1, x.shape[1]
    out = np.zeros((Bn, C))
    gx = np.zeros(xd.shape, dtype=xd.dtype)
    for b in range(Bn):
        lo, hi = ptr[b], ptr[b + 1]
        if hi == lo:
            continue
        scale = 1.0 / (hi - lo) if reduce == 'mean' else 1.0
        out[b] = v[lo:hi].sum(0) * scale
        if g is not None:
            if soft_abs:
                gx[lo:hi] = np.where(org[lo:hi], 0.0, g[b][None, :] * scale * xd[lo:hi] / np.where(org[lo:hi], 1.0, v[lo:hi]))
            else:
                gx[lo:hi] = g[b][None, :] * scale
    return out, gx


POOL_SIZES = (0, 1, 20000, 5, 300, 0, 64, 65)          # an empty mesh first and in the middle, one vertex, 20 000 next to 5


def _pool_input(C, soft_abs, dtype, seed):
    rng = np.random.default_rng(seed)
    N = sum(POOL_SIZES)
    if soft_abs:
        x = rng.standard_normal((N, C)) + 1j * rng.standard_normal((N, C))
        x[3, 0] = 0
        x[7, :] = 0
        x[20001 + 2, C - 1] = complex(5e-8, -5e-8)              # inside the origin box
        x[11, 0] = complex(5e-8, 0.0)
        x[12, 0] = complex(2e-7, 5e-8)                          # outside: one component beyond the box
        x[13, 0] = complex(-1e-7, 0.0) if dtype == 'f64' else complex(float(np.float32(-1e-7)), 0.0)      # on the edge: not inside (strict <)
        x = x.astype(np.complex64 if dtype == 'f32' else np.complex128)
    else:
        x = rng.standard_normal((N, C)).astype(np.float32 if dtype == 'f32' else np.float64)
    ptr = np.concatenate(([0], np.cumsum(POOL_SIZES))).astype(np.int64)
    return x, ptr


@pytest.mark.parametrize('dtype', ['f32', 'f64'])
@pytest.mark.parametrize('soft_abs', [True, False], ids=['softabs', 'real'])
@pytest.mark.parametrize('reduce', ['mean', 'sum'])
@pytest.mark.parametrize('C', [1, 3, 16, 48, 130])
def test_mesh_pool_equals_float64_restatement(C, reduce, soft_abs, dtype, dev):
    from fieldconv_amd.pooling import mesh_pool
    x, ptr = _pool_input(C, soft_abs, dtype, seed=C)
    g = np.random.default_rng(C + 1).standard_normal((len(ptr) - 1, C))
    xd = D(x, dev).requires_grad_(True)
    ptr_d = D(ptr, dev)
    out = mesh_pool(xd, ptr_d, reduce, soft_abs)
    gd = D(g.astype(np.float32 if dtype == 'f32' else np.float64), dev)
    gx, = torch.autograd.grad(out, [xd], grad_outputs=gd)
    ref, gref = pool_ref(x, ptr, reduce, soft_abs, H(gd).astype(np.float64))
    gate = TOL if dtype == 'f32' else 1e-12
    e_out, e_gx = rel_err(H(out), ref), rel_err(H(gx), gref)
    print('%s C=%d %s %s: out %.1e, gx %.1e' % (dtype, C, reduce, 'softabs' if soft_abs else 'real', e_out, e_gx))
    assert out.dtype == (torch.float32 if dtype == 'f32' else torch.float64) and out.shape == (len(ptr) - 1, C)
    assert e_out < gate and e_gx < gate
    # empty meshes: exactly 0; entries inside the origin box: gradient exactly 0
    o = H(out)
    assert np.all(o[0] == 0) and np.all(o[5] == 0)
    if soft_abs:
        gxh = H(gx)
        for n, c in ((3, 0), (7, C - 1), (20003, C - 1), (11, 0)):
            assert gxh[n, c] == 0
        assert gxh[12, 0] != 0 and gxh[13, 0] != 0
    # two runs, the same bits
    out2 = mesh_pool(xd, ptr_d, reduce, soft_abs)
    gx2, = torch.autograd.grad(out2, [xd], grad_outputs=gd)
    assert torch.equal(out, out2) and torch.equal(torch.view_as_real(gx) if soft_abs else gx, torch.view_as_real(gx2) if soft_abs else gx2)
    # a host ptr gives the same result
    assert torch.equal(mesh_pool(xd, torch.from_numpy(ptr), reduce, soft_abs), out)


def test_mesh_pool_module_and_mesh_mean(dev):
    from fieldconv_amd.functional import mesh_mean
    from fieldconv_amd.nn import MeshPool
    x, ptr = _pool_input(5, True, 'f32', seed=1)
    xd, ptr_d = D(x, dev), D(ptr, dev)
    out = MeshPool()(xd, ptr_d)
    assert rel_err(H(out), pool_ref(x, ptr, 'mean', True)[0]) < TOL
    assert rel_err(H(MeshPool(reduce='sum')(xd, ptr_d)), pool_ref(x, ptr, 'sum', True)[0]) < TOL
    v = np.random.default_rng(0).standard_normal(x.shape[0]).astype(np.float32)
    got = mesh_mean(D(v, dev), ptr_d)
    assert got.shape == (len(ptr) - 1,)
    assert rel_err(H(got), pool_ref(v[:, None], ptr, 'mean', False)[0][:, 0]) < TOL
    assert torch.equal(mesh_mean(D(v, dev)[:, None], ptr_d)[:, 0], got)
    # the read-out of one mesh is the classification networks' mean(softAbs(x), dim=0)
    from fieldconv_amd.utils.field import softAbs
    one = torch.tensor([0, x.shape[0]])
    assert rel_err(H(MeshPool()(xd, one)), H(torch.mean(softAbs(xd), dim=0, keepdim=True))) < TOL


def test_mesh_pool_gradcheck_float64(dev):
    from fieldconv_amd.pooling import mesh_pool
    gen = torch.Generator().manual_seed(3)
    ptr = torch.tensor([0, 3, 3, 70, 75], device=dev)
    x = torch.complex(torch.randn(75, 3, generator=gen, dtype=torch.float64), torch.randn(75, 3, generator=gen, dtype=torch.float64))
    x = x.to(dev).requires_grad_(True)
    r = torch.randn(75, 3, generator=gen, dtype=torch.float64).to(dev).requires_grad_(True)
    for reduce in ('mean', 'sum'):
        assert torch.autograd.gradcheck(lambda t: mesh_pool(t, ptr, reduce, True), (x,))
        assert torch.autograd.gradcheck(lambda t: mesh_pool(t, ptr, reduce, False), (r,))


def test_mesh_pool_writes_inside_its_buffers(dev, monkeypatch):
    """Output, workspace and gradient carved out of guarded allocations, as tests/test_gpu_canary.py does for the other entry points."""
    from test_gpu_canary import GuardedTorch
    import fieldconv_amd._launch as launch
    import fieldconv_amd.pooling as pooling
    guarded = GuardedTorch()
    monkeypatch.setattr(pooling, 'torch', guarded)
    monkeypatch.setattr(launch, 'torch', guarded)
    n = 0
    for C in (1, 48, 130):
        for soft_abs, dtype in ((True, 'f32'), (False, 'f32'), (True, 'f64'), (False, 'f64')):
            x, ptr = _pool_input(C, soft_abs, dtype, seed=9)
            xd = D(x, dev).requires_grad_(True)
            out = pooling.mesh_pool(xd, D(ptr, dev), 'mean', soft_abs)
            torch.autograd.grad(out, [xd], grad_outputs=torch.ones_like(out))
            n += guarded.check(f'mesh_pool C={C} softabs={soft_abs} {dtype}')
    assert n >= 36


def test_pooling_argument_errors_raise_before_any_launch(dev, monkeypatch):
    from fieldconv_amd import _lib
    from fieldconv_amd.functional import mesh_mean
    from fieldconv_amd.nn import MeshPool
    from fieldconv_amd.transforms import farthest_point_sample_batched, radius_edges_batched

    def no_device(*a, **k):
        raise AssertionError('device work attempted')
    monkeypatch.setattr(_lib, 'load', no_device)
    x = torch.zeros(10, 4, dtype=torch.complex64, device=dev)
    pool = MeshPool()
    for bad in ([0, 6, 4, 10], [0, 4, 9], [1, 4, 10], [0, 11, 10]):
        for where in (dev, 'cpu'):
            with pytest.raises(ValueError):
                pool(x, torch.tensor(bad, device=where))
            with pytest.raises(ValueError):
                mesh_mean(x.real.contiguous(), torch.tensor(bad, device=where))
    with pytest.raises(ValueError):
        pool(x, torch.tensor([0, 10], dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        pool(x.real.contiguous(), torch.tensor([0, 10], device=dev))          # soft_abs wants complex features
    with pytest.raises(ValueError):
        MeshPool(reduce='max')
    with pytest.raises(RuntimeError):
        pool(x.cpu(), torch.tensor([0, 10]))
    with pytest.raises(RuntimeError):
        mesh_mean(torch.zeros(10, 1), torch.tensor([0, 10]))
    pos = torch.rand(10, 3, device=dev)
    for bad in ([0, 6, 4, 10], [0, 4, 9]):
        with pytest.raises(ValueError):
            farthest_point_sample_batched(pos, torch.tensor(bad), 1)
        with pytest.raises(ValueError):
            radius_edges_batched(pos, torch.tensor(bad), 0.1)
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 10]), 5)          # mesh 0 has four points
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 10]), [2, 7])
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 10]), 2, start=[0, 6])
    with pytest.raises(ValueError):
        radius_edges_batched(pos, torch.tensor([0, 4, 10]), -1.0)


# ---------------------------------------------------------------- batched FPS / radius: the restatements of test_gpu_support_graph.py
def sq_dist(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps_ref(p, S, start):
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = p.shape[0]
    mind = np.full(N, np.inf, dtype=np.float32)
    taken = np.zeros(N, dtype=bool)
    out = np.empty(S, dtype=np.int64)
    last = start
    for k in range(S):
        out[k] = last
        taken[last] = True
        if k + 1 == S:
            break
        np.minimum(mind, sq_dist(p, p[last]), out=mind)
        last = int(np.argmax(np.where(taken, np.float32(-1), mind)))        # first maximum: the lowest index
    return out


def _truncate(q, n, d2, K):
    order = np.lexsort((n, d2, q))
    q, n = q[order], n[order]
    first = np.searchsorted(q, q, side='left')
    keep = (np.arange(q.size) - first) < K
    q, n = q[keep], n[keep]
    order = np.lexsort((n, q))
    return np.stack((q[order], n[order]), 1).astype(np.int64)


def radius_ref(p, eps, K):
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(p, dtype=np.float32)
    N = p.shape[0]
    r2 = np.float32(eps) * np.float32(eps)
    if N <= 3000:
        d2 = sq_dist(p[None, :, :], p[:, None, :])
        q, n = np.nonzero(d2 < r2)
        return _truncate(q, n, d2[q, n], K)
    tree = cKDTree(p.astype(np.float64))
    pairs = tree.query_pairs(float(np.sqrt(np.float64(r2))) * (1 + 1e-4) + 1e-7, output_type='ndarray')
    q = np.concatenate((pairs[:, 0], pairs[:, 1], np.arange(N)))
    n = np.concatenate((pairs[:, 1], pairs[:, 0], np.arange(N)))
    d2 = sq_dist(p[n], p[q])
    m = d2 < r2
    return _truncate(q[m], n[m], d2[m], K)


SETS = (1, 2, 700, 5000, 17000, 333)          # 17 000 > 16 384: the workspace path of the sampling kernel


def _point_sets():
    sets = [np.random.default_rng(40 + i).random((n, 3)).astype(np.float32) for i, n in enumerate(SETS)]
    sets[2][350:700] = sets[2][:350]                    # every position of this set twice
    sets[5][17] = (50.0, 50.0, 50.0)                    # an isolated point
    ptr = np.concatenate(([0], np.cumsum(SETS))).astype(np.int64)
    return sets, ptr


def test_batched_fps_equals_restatement_and_single_calls(dev):
    from fieldconv_amd.transforms import farthest_point_sample, farthest_point_sample_batched
    sets, ptr = _point_sets()
    pos = D(np.concatenate(sets), dev)
    S = [1, 2, 450, 512, 1024, 333]
    starts = [0, 1, 3, 4999, 16999, 100]
    got = farthest_point_sample_batched(pos, D(ptr, dev), S, starts)
    assert got.device == dev and got.dtype == torch.int64 and got.shape == (sum(S),)
    again = farthest_point_sample_batched(pos, torch.from_numpy(ptr), S, starts)          # a host ptr; two runs, the same indices
    assert torch.equal(got, again)
    got = got.cpu().numpy()
    o = 0
    for b, p in enumerate(sets):
        mine = got[o:o + S[b]]
        o += S[b]
        assert np.array_equal(mine, fps_ref(p, S[b], starts[b])), b
        assert np.array_equal(mine, farthest_point_sample(D(p, dev), S[b], starts[b]).cpu().numpy()), b
        assert np.unique(mine).size == S[b]
    # one n_samples / start for all sets
    same = farthest_point_sample_batched(pos[int(ptr[2]):], D(ptr[2:] - ptr[2], dev), 300).cpu().numpy()
    for j, b in enumerate(range(2, 6)):
        assert np.array_equal(same[300 * j:300 * (j + 1)], fps_ref(sets[b], 300, 0)), b


@pytest.mark.parametrize('eps,K', [(0.07, 512), (0.07, 8), (0.3, 40)])
def test_batched_radius_equals_restatement_per_mesh(eps, K, dev):
    from fieldconv_amd.transforms import radius_edges, radius_edges_batched
    sets, ptr = _point_sets()
    if eps > 0.1:
        sets, ptr = sets[:4], ptr[:5]                   # (a wide radius: the small sets and 5 000 points, most queries overfull)
    pos = D(np.concatenate(sets), dev)
    got = radius_edges_batched(pos, D(ptr, dev), eps, K)
    assert got.device == dev and got.dtype == torch.int64 and got.dim() == 2 and got.shape[1] == 2
    ref = np.concatenate([radius_ref(p, eps, K) + ptr[b] for b, p in enumerate(sets)])
    got = got.cpu().numpy()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.array_equal(got, ref)
    single = np.concatenate([radius_edges(D(p, dev), eps, K).cpu().numpy() + ptr[b] for b, p in enumerate(sets)])
    assert np.array_equal(got, single)
    if len(sets) == 6 and K == 512:
        iso = int(ptr[5]) + 17
        assert np.array_equal(got[got[:, 0] == iso], [[iso, iso]])          # the isolated point: only itself
    if K == 8:
        assert np.bincount(got[:, 0]).max() == 8                           # the truncation bites
    # an empty set in the middle changes nothing but the numbering
    ptr_e = np.concatenate((ptr[:3], ptr[2:]))
    assert np.array_equal(radius_edges_batched(pos, D(ptr_e, dev), eps, K).cpu().numpy(), got)


def sphere_points(N, seed=0, jitter=0.15):
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / N
    rad = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    lon = math.pi * (3.0 - math.sqrt(5.0)) * i
    p = np.stack((rad * np.cos(lon), rad * np.sin(lon), z), 1)
    p = p + (jitter / math.sqrt(N)) * np.random.default_rng(seed).standard_normal((N, 3))
    return (p / np.linalg.norm(p, axis=1, keepdims=True)).astype(np.float32)


def test_support_graph_on_a_batch_feeds_fcprecomp_and_fieldconv(dev):
    """SupportGraph on a MeshBatch of three point sets: mesh for mesh the single-mesh transform plus offsets; then a closed-form log
    map on the union's edges, FCPrecomp on the batch and one FieldConv forward against the oracle."""
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.data.synthetic import _edge_fields, _frames
    from fieldconv_amd.nn import FieldConv
    from fieldconv_amd.transforms import FCPrecomp, SupportGraph
    from oracle.torch_composites import FCPrecomp as FCPrecompRef
    sizes, eps, Bl, R, I, O = (1500, 2200, 900), 0.16, 2, 6, 16, 16
    sets = [torch.from_numpy(sphere_points(n, seed=30 + i)) for i, n in enumerate(sizes)]
    batch = SupportGraph(eps, sample_n=600, generator=torch.Generator().manual_seed(4))(MeshBatch.from_list([Data(pos=p) for p in sets]))
    gen = torch.Generator().manual_seed(4)
    pp, vp = batch.pos_ptr.tolist(), batch.ptr.tolist()
    assert vp == [0, 600, 1200, 1800] and batch.batch.tolist() == [0] * 600 + [1] * 600 + [2] * 600
    ep = batch.edge_ptr.tolist()
    for b, p in enumerate(sets):
        one = SupportGraph(eps, sample_n=600, generator=gen)(Data(pos=p.clone()))          # the same generator state: one draw per mesh, in order
        assert torch.equal(batch.sample_idx[vp[b]:vp[b + 1]], one.sample_idx + pp[b]), b
        assert torch.equal(batch.supp_edges[ep[b]:ep[b + 1]], one.supp_edges + vp[b]), b
        m = batch.mesh(b)
        assert torch.equal(m.sample_idx, one.sample_idx) and torch.equal(m.supp_edges, one.supp_edges)
    assert ep[-1] == batch.supp_edges.shape[0]
    # sample_n above a mesh's size keeps every point of that mesh
    small = SupportGraph(0.3, sample_n=1000, max_num_neighbors=12, random_start=False)(MeshBatch.from_list([Data(pos=p) for p in sets]))
    assert small.ptr.tolist() == [0, 1000, 2000, 2900]
    assert torch.equal(small.sample_idx[2000:], torch.arange(900) + small.pos_ptr[2])
    # closed-form log map and transport on the union's edges (all of them inside one mesh), then the product path
    pts = batch.pos[batch.sample_idx].numpy().astype(np.float64)
    pts /= np.linalg.norm(pts, axis=1, keepdims=True)
    s, t = batch.supp_edges[:, 0].numpy(), batch.supp_edges[:, 1].numpy()
    assert np.array_equal(np.searchsorted(vp, s, side='right'), np.searchsorted(vp, t, side='right'))
    e1, e2 = _frames(pts)
    dist, ang, xp_ang = _edge_fields(pts[s], e1[s], e2[s], pts[t], e1[t], e2[t])
    M = pts.shape[0]
    batch.logMag, batch.logAng = torch.from_numpy(dist).float(), torch.from_numpy(ang).float()
    batch.xp = torch.polar(torch.ones(dist.size), torch.from_numpy(xp_ang).float())
    batch.w = torch.full((M, 1), 4 * math.pi / 600)
    eps_g = float(dist.max()) * 1.0001
    ref_edges, ref_sten, _, _ = FCPrecompRef(Bl, R, eps_g)(batch)
    e_dev, sten_dev, _, _ = FCPrecomp(Bl, R, eps_g)(batch.to(dev))
    assert torch.equal(e_dev.cpu(), ref_edges)
    g = torch.Generator().manual_seed(5)
    x = torch.complex(torch.randn(M, I, generator=g), torch.randn(M, I, generator=g))
    conv = FieldConv(I, O, band_limit=Bl, n_rings=R, ftype=1).to(dev)
    y = conv(x.to(dev), e_dev, sten_dev)
    W = orc.effective_filter(H(conv.zonal), H(conv.spherical), H(conv.phase), 1, Bl)
    y_ref = orc.fieldconv_forward(x.numpy(), ref_edges.numpy(), ref_sten.numpy(), W)
    assert rel_err(H(y), y_ref) < TOL
