"""The fused classification head on the device (fieldconv_amd.head, csrc/fc_linear_ce.hip) against the float64 restatement
(tests/_head_ref.py).

Accuracy gate.  Not a fixed number: torch's own float32 composite (`cross_entropy(linear(h, W, b), target)`, or the dense
label-smoothing formula) runs on the same device on the same inputs, and its distance to float64 is the yardstick -- the fused
kernels do the same float32 arithmetic with sums in another order, which earns a small multiple (4 x), not an order of
magnitude.  Floor: 1e-6 of the reference tensor's largest entry.  Errors are max |a - ref|.  Measured on an MI355X: README.

Tiles are 64 rows x 64 classes, H goes through LDS in chunks of 32 and g_h / g_W are held 256 columns at a time, so the shapes
sit under, at and over 64 (rows, classes), 32 and 256 (H), with ragged tails everywhere."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _head_ref as href
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

REDUCED = os.environ.get('FC_MFMA') == 'f16'
SHAPES = [(1, 1, 1), (3, 5, 2), (17, 7, 33), (64, 256, 64), (65, 256, 129), (130, 260, 517), (257, 64, 4999), (63, 31, 63), (128, 33, 65)]
PARTS = [0, 1, 3]
IGNORE = -100


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def D(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def Hn(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def inputs(N, H, K):
    """h ~ N(0,1); W ~ N(0,1/H) with one class row scaled by 150 (its logits reach beyond +-100: exp overflows in float32 without
    the running maximum) and, for K > 3, class 3 a copy of class 1 (exact ties in every row); one row of h zero (its logits are
    the bias alone); targets with class 0 and class K - 1 and some ignore_index rows."""
    rng = np.random.default_rng(1000 * N + 10 * H + K)
    h = rng.standard_normal((N, H)).astype(np.float32)
    W = (rng.standard_normal((K, H)) / np.sqrt(H)).astype(np.float32)
    W[K // 2] *= 150
    b = rng.standard_normal(K).astype(np.float32)
    if K > 3:
        W[3], b[3] = W[1], b[1]
    if N > 4:
        h[4] = 0
    target = rng.integers(0, K, N)
    target[0] = 0
    if N > 1:
        target[1] = K - 1
    if N > 2:
        target[2::7] = IGNORE
    up = rng.standard_normal(N).astype(np.float32)
    return h, W, b, target, up


CONFIGS = {'mean': ('mean', 0.0), 'none_smooth': ('none', 0.1), 'sum': ('sum', 0.0)}


@functools.lru_cache(maxsize=None)
def reference(N, H, K, config):
    """float64 restatement, computed once per shape and configuration and never modified"""
    h, W, b, target, up = inputs(N, H, K)
    reduction, smoothing = CONFIGS[config]
    out = href.head(h, W, b, target, reduction, smoothing, IGNORE, upstream=up if reduction == 'none' else None)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def composite(ht, Wt, bt, tt, reduction, smoothing):
    """torch's own float32 way on the device, logits materialised"""
    z = torch.nn.functional.linear(ht, Wt, bt)
    if smoothing == 0:
        return torch.nn.functional.cross_entropy(z, tt, reduction=reduction, ignore_index=IGNORE)
    K = z.shape[1]
    counted = tt != IGNORE
    q = torch.full_like(z, smoothing / (K - 1))
    q[torch.arange(z.shape[0], device=z.device), tt.clamp(min=0)] = 1.0 - smoothing
    rows = -(q * torch.log_softmax(z, 1)).sum(1) * counted
    return rows if reduction == 'none' else (rows.sum() if reduction == 'sum' else rows.sum() / counted.sum())


def run(fn, h, W, b, target, up, reduction, dev):
    ht, Wt, bt = (D(a, dev).requires_grad_(True) for a in (h, W, b))
    loss = fn(ht, Wt, bt, D(target, dev))
    grads = torch.autograd.grad(loss, [ht, Wt, bt], grad_outputs=D(up, dev) if reduction == 'none' else None)
    return [loss.detach()] + list(grads)


@functools.lru_cache(maxsize=None)
def composite_errors(N, H, K, config):
    dev = torch.device('cuda:0')
    reduction, smoothing = CONFIGS[config]
    h, W, b, target, up = inputs(N, H, K)
    got = run(lambda *a: composite(*a, reduction, smoothing), h, W, b, target, up, reduction, dev)
    return [float(np.max(np.abs(Hn(g).astype(np.float64) - r))) for g, r in zip(got, reference(N, H, K, config))]


def gates(N, H, K, config):
    ref = reference(N, H, K, config)
    return [4 * max(e, 1e-6 * float(np.max(np.abs(r)))) for e, r in zip(composite_errors(N, H, K, config), ref)]


# (label smoothing needs two classes: the one-class shape runs the unsmoothed configurations only)
LOSS_CASES = [pytest.param(s, c, id='x'.join(map(str, s)) + '-' + c) for s in SHAPES for c in CONFIGS if not (CONFIGS[c][1] > 0 and s[2] < 2)]


@pytest.mark.parametrize('parts', PARTS)
@pytest.mark.parametrize('shape,config', LOSS_CASES)
def test_loss_and_gradients_against_float64(dev, shape, parts, config):
    from fieldconv_amd.functional import linear_cross_entropy
    N, H, K = shape
    reduction, smoothing = CONFIGS[config]
    h, W, b, target, up = inputs(N, H, K)
    ref = reference(N, H, K, config)

    def fused(ht, Wt, bt, tt):
        return linear_cross_entropy(ht, Wt, bt, tt, reduction, smoothing, IGNORE, parts)
    got = run(fused, h, W, b, target, up, reduction, dev)
    again = run(fused, h, W, b, target, up, reduction, dev)
    errs = [float(np.max(np.abs(Hn(g).astype(np.float64) - r))) for g, r in zip(got, ref)]
    gate = gates(N, H, K, config)
    print('%s parts %d %s: errors (loss, g_h, g_W, g_b) fused %s, composite %s, gate %s' % (
        shape, parts, config, ['%.2e' % e for e in errs], ['%.2e' % e for e in composite_errors(N, H, K, config)], ['%.2e' % g for g in gate]))
    for name, e, g in zip(('loss', 'g_h', 'g_W', 'g_b'), errs, gate):
        assert e <= g, (name, e, g)
    for a, c in zip(got, again):          # two runs: the same bits
        assert torch.equal(a, c)
    if reduction == 'none':               # ignored rows: exactly zero, loss and gradient
        ign = np.nonzero(target == IGNORE)[0]
        assert (Hn(got[0])[ign] == 0).all() and (Hn(got[1])[ign] == 0).all()


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_parts_agree_and_mean_is_the_rows_summed(dev, shape):
    from fieldconv_amd.functional import linear_cross_entropy
    N, H, K = shape
    h, W, b, target, up = inputs(N, H, K)
    gate = gates(N, H, K, 'mean')
    one, three = (run(lambda *a: linear_cross_entropy(*a, 'mean', 0.0, IGNORE, p), h, W, b, target, up, 'mean', dev) for p in (1, 3))
    for name, a, c, g in zip(('loss', 'g_h', 'g_W', 'g_b'), one, three, gate):
        assert float((a - c).abs().max()) <= g, name
    for p, mean in ((1, one[0]), (3, three[0])):          # 'mean' / 'sum' are the rows of 'none' added in index order in double
        rows = Hn(linear_cross_entropy(D(h, dev), D(W, dev), D(b, dev), D(target, dev), 'none', parts=p))
        assert abs(float(mean) - href.reduce_rows(rows, target, 'mean', IGNORE)) <= gate[0]
        total = float(linear_cross_entropy(D(h, dev), D(W, dev), D(b, dev), D(target, dev), 'sum', parts=p))
        assert abs(total - href.reduce_rows(rows, target, 'sum', IGNORE)) <= gates(N, H, K, 'sum')[0]


@functools.lru_cache(maxsize=None)
def kernel_logits(N, H, K):
    """All N x K logits as the KERNEL rounds them, eight classes at a time: linear_topk(k=8) of a slice of eight classes returns
    every one of its logits.  (That a logit does not depend on the tile or slice it is computed in is the design rule.)"""
    from fieldconv_amd.functional import linear_topk
    dev = torch.device('cuda:0')
    h, W, b, _, _ = inputs(N, H, K)
    ht, Wt, bt = D(h, dev), D(W, dev), D(b, dev)
    z = torch.empty((N, K), dtype=torch.float32, device=dev)
    for c in range(0, K, 8):
        idx, zk = linear_topk(ht, Wt[c:c + 8], bt[c:c + 8], k=8)
        n = min(8, K - c)
        z[:, c:c + n] = torch.gather(zk[:, :n], 1, torch.argsort(idx[:, :n], 1))
    out = Hn(z)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize('parts', PARTS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_topk_equals_restatement_on_the_kernels_logits(dev, shape, parts):
    from fieldconv_amd.functional import linear_logsumexp, linear_topk
    from fieldconv_amd.nn import vertex_accuracy
    N, H, K = shape
    h, W, b, target, _ = inputs(N, H, K)
    ht, Wt, bt = D(h, dev), D(W, dev), D(b, dev)
    z = kernel_logits(N, H, K)
    assert rel_err(z.astype(np.float64), href.logits(h, W, b)) < 1e-5
    lse = Hn(linear_logsumexp(ht, Wt, bt, parts))
    for k in (1, 3, 8):
        idx, zk = linear_topk(ht, Wt, bt, k, parts)
        want_idx, want_z = href.topk(z, k)
        assert idx.dtype == torch.int64 and zk.dtype == torch.float32
        assert np.array_equal(Hn(idx), want_idx)
        assert np.array_equal(Hn(zk).view(np.uint32), want_z.view(np.uint32))          # bit for bit the logits the kernels see
        if k > K:
            assert (Hn(idx)[:, K:] == -1).all() and np.isneginf(Hn(zk)[:, K:]).all()
        assert (lse >= Hn(zk)[:, 0]).all()
        acc = vertex_accuracy(idx, D(target, dev))
        assert np.array_equal(Hn(acc), href.accuracy(want_idx, target, IGNORE))
    if K > 3:          # class 3 copies class 1: an exact tie, and the lower class comes first
        idx8 = Hn(linear_topk(ht, Wt, bt, 8, parts)[0])
        both = [(list(r).index(1), list(r).index(3)) for r in idx8 if 1 in r and 3 in r]
        assert (z[:, 1] == z[:, 3]).all() and all(p3 == p1 + 1 for p1, p3 in both) and (K > 8 or len(both) == N)
    # the loss sees the same logits: per-row loss = lse - z[target], to the rounding of one subtraction
    from fieldconv_amd.functional import linear_cross_entropy
    rows = Hn(linear_cross_entropy(ht, Wt, bt, D(target, dev), 'none', parts=parts))
    ok = target != IGNORE
    want = lse[ok] - z[ok, target[ok]]
    assert np.array_equal(rows[ok].view(np.uint32), want.astype(np.float32).view(np.uint32))


@pytest.mark.parametrize('parts', [1, 3])
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 8])
def test_topk_every_rung_of_the_list_ladder(dev, k, parts):
    """Every list length the kernels are compiled for (1, 2, 4, 8), filled (k = K) and not (k = 3, 5), from one part and merged
    from three.  65 rows and 130 classes: a second row tile, and three class tiles, so that each of three parts has one."""
    from fieldconv_amd.functional import linear_topk
    N, H, K = 65, 33, 130
    h, W, b, _, _ = inputs(N, H, K)
    idx, zk = linear_topk(D(h, dev), D(W, dev), D(b, dev), k, parts)
    want_idx, want_z = href.topk(kernel_logits(N, H, K), k)
    assert np.array_equal(Hn(idx), want_idx)
    assert np.array_equal(Hn(zk).view(np.uint32), want_z.view(np.uint32))


def test_equal_logits_nan_logits_and_bad_targets(dev):
    from fieldconv_amd.functional import linear_cross_entropy, linear_topk
    N, H, K = 70, 9, 130
    h, W, b, target, _ = inputs(N, H, K)
    ht, tt = D(h, dev), D(target, dev)
    # all logits equal (zero weights, constant bias): loss log K, prediction the lowest classes
    Wz, bc = torch.zeros((K, H), device=dev), torch.full((K,), 0.37, device=dev)
    rows = Hn(linear_cross_entropy(ht, Wz, bc, tt, 'none'))
    ok = target != IGNORE
    assert np.abs(rows[ok] - np.log(K)).max() < 4e-6 * np.log(K) + 1e-6          # log and the sum of K ones in float32
    idx, zk = linear_topk(ht, Wz, bc, 8)
    assert (Hn(idx) == np.arange(8)).all() and (Hn(zk) == np.float32(0.37)).all()
    # a NaN class sorts after every number, and makes the losses NaN
    Wn = D(W, dev).clone()
    Wn[5] = float('nan')
    idx, zk = linear_topk(ht[:, :], Wn[:8].contiguous(), D(b[:8], dev), 8)
    assert (Hn(idx)[:, 7] == 5).all() and np.isnan(Hn(zk)[:, 7]).all() and np.isfinite(Hn(zk)[:, :7]).all()
    assert np.isnan(Hn(linear_cross_entropy(ht, Wn, D(b, dev), tt, 'none'))[ok]).all()
    # a target outside [0,K) that is not ignore_index: that row's loss is NaN, the others are untouched; its gradients NaN
    for bad in (K, -1, 2 ** 40):
        tb = target.copy()
        tb[6] = bad
        hg, Wg = D(h, dev).requires_grad_(True), D(W, dev).requires_grad_(True)
        rows_b = linear_cross_entropy(hg, Wg, D(b, dev), D(tb, dev), 'none')
        good = Hn(linear_cross_entropy(ht, D(W, dev), D(b, dev), tt, 'none'))
        got = Hn(rows_b)
        assert np.isnan(got[6]) and np.array_equal(np.delete(got, 6), np.delete(good, 6))
        g_h, g_W = torch.autograd.grad(rows_b, [hg, Wg], grad_outputs=torch.ones_like(rows_b))
        assert np.isnan(Hn(g_h)[6]).all() and np.isfinite(np.delete(Hn(g_h), 6, 0)).all() and np.isnan(Hn(g_W)).all()
    every = torch.full((N,), IGNORE, dtype=torch.int64, device=dev)
    assert np.isnan(float(linear_cross_entropy(ht, D(W, dev), D(b, dev), every))) and float(linear_cross_entropy(ht, D(W, dev), D(b, dev), every, 'sum')) == 0


def test_gradients_nobody_asked_for_are_not_launched(dev, monkeypatch):
    from fieldconv_amd import _lib
    from fieldconv_amd.functional import linear_cross_entropy
    N, H, K = 65, 33, 129
    h, W, b, target, _ = inputs(N, H, K)
    lib = _lib.load()
    calls = {}
    for name in ('fc_linear_ce_backward_input', 'fc_linear_ce_backward_weight'):
        def counted(*a, _fn=getattr(lib, name), _name=name):
            calls[_name] = calls.get(_name, 0) + 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, counted)
    ref = href.head(h, W, b, target, 'mean', 0.0, IGNORE)
    for need in ((True, False, False), (False, True, True), (False, False, True), (True, True, False)):
        calls.clear()
        ts = [D(a, dev).requires_grad_(r) for a, r in zip((h, W, b), need)]
        loss = linear_cross_entropy(*ts, D(target, dev))
        loss.backward()
        assert [t.grad is not None for t in ts] == list(need)
        assert calls.get('fc_linear_ce_backward_input', 0) == int(need[0]) and calls.get('fc_linear_ce_backward_weight', 0) == int(need[1] or need[2])
        for t, r in zip(ts, ref[1:]):
            if t.grad is not None:          # (the right tensor in the right place; accuracy is gated above)
                assert rel_err(Hn(t.grad), r) < 1e-4
    # no bias at all
    hg = D(h, dev).requires_grad_(True)
    loss = linear_cross_entropy(hg, D(W, dev), None, D(target, dev))
    want = href.head(h, W, None, target, 'mean', 0.0, IGNORE)
    assert rel_err(Hn(loss), want[0]) < 1e-5 and rel_err(Hn(torch.autograd.grad(loss, hg)[0]), want[1]) < 1e-4


def test_mesh_batch_per_mesh_means(dev):
    """three meshes of 40-150 vertices in one MeshBatch-style range table: the per-mesh means of the per-row losses equal the
    per-mesh losses computed mesh by mesh (float32 means of at most 150 terms: 150 eps ~ 1e-5 relative covers any order)"""
    from fieldconv_amd.functional import linear_cross_entropy, mesh_mean
    sizes, H, K = (40, 150, 97), 48, 150
    N = sum(sizes)
    rng = np.random.default_rng(7)
    h, W, b = (rng.standard_normal(s).astype(np.float32) for s in ((N, H), (K, H), (K,)))
    W = (W / np.sqrt(H)).astype(np.float32)
    target = rng.integers(0, K, N)
    ptr = torch.tensor(np.concatenate(([0], np.cumsum(sizes))), dtype=torch.int64, device=dev)
    ht, Wt, bt, tt = D(h, dev), D(W, dev), D(b, dev), D(target, dev)
    batched = mesh_mean(linear_cross_entropy(ht, Wt, bt, tt, reduction='none')[:, None], ptr).mean()
    lo, acc = 0, 0.0
    for n in sizes:
        acc += float(linear_cross_entropy(ht[lo:lo + n], Wt, bt, tt[lo:lo + n]))
        lo += n
    assert abs(float(batched) - acc / 3) <= 1e-5 * abs(acc / 3)
    want = np.mean([href.head(h[a:c], W, b, target[a:c])[0] for a, c in zip(np.cumsum((0,) + sizes[:-1]), np.cumsum(sizes))])
    assert abs(float(batched) - want) <= 1e-5 * abs(want)


def test_no_write_outside_any_buffer(dev, monkeypatch):
    """Guard bands as in tests/test_gpu_canary.py: every buffer the head allocates (outputs, lse, workspaces, gradients) is carved
    out of a larger allocation whose margins hold a byte pattern; ragged N, H, K, parts 0 / 1 / 3."""
    import fieldconv_amd._launch as launch
    import fieldconv_amd.head as head
    from test_gpu_canary import GuardedTorch
    g = GuardedTorch()
    monkeypatch.setattr(head, 'torch', g)
    monkeypatch.setattr(launch, 'torch', g)
    N, H, K = 131, 37, 203
    h, W, b, target, _ = inputs(N, H, K)
    n = 0
    for parts in PARTS:
        ts = [D(a, dev).requires_grad_(True) for a in (h, W, b)]
        loss = head.linear_cross_entropy(*ts, D(target, dev), 'mean', 0.1, IGNORE, parts)
        torch.autograd.grad(loss, ts)
        head.linear_topk(*[t.detach() for t in ts], 8, parts)
        n += g.check('linear_cross_entropy / linear_topk, parts %d' % parts)
    assert n >= 3 * 9


@pytest.mark.skipif(REDUCED, reason='twenty-five layers deep: checks the fp32-grade path')
def test_correspondence_net_golden_with_the_fused_head(dev):
    """tests/test_gpu_parity.py::test_correspondence_net_golden with lin2 + cross_entropy replaced by LinearCrossEntropy loaded
    from the network's lin2: the loss and every recorded parameter-gradient sample meet that test's own gates."""
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock, LinearCrossEntropy, TangentPerceptron
    from fieldconv_amd.transforms import FCPrecomp
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden'))
    from param_fill import fill_params, grad_sample
    c = load_golden('net_correspondence.npz')['correspondence_net']
    B, R, nf = int(c['B']), int(c['R']), int(c['nf'])
    kw = dict(band_limit=B, n_rings=R, ftype=1)
    mods = torch.nn.ModuleDict(dict(
        lift=LiftBlock(3, 16, n_rings=R, ftype=1),
        resnet1=FCResNetBlock(16, nf, **kw), resnet2=FCResNetBlock(nf, nf, **kw), resnet3=FCResNetBlock(nf, nf, **kw),
        resnet4=FCResNetBlock(nf, nf, **kw), resnet5=FCResNetBlock(nf, nf, **kw), resnet6=FCResNetBlock(nf, nf, **kw),
        resnet7=FCResNetBlock(nf, nf, **kw), resnet8=FCResNetBlock(nf, 16, frontload=True, **kw),
        echo=ECHOBlock(16, nf, n_des=int(c['n_des']), n_bins=int(c['n_bins']), **kw),
        res1=TangentPerceptron(16, nf), res2=TangentPerceptron(nf, nf), res3=TangentPerceptron(nf, nf),
        res4=TangentPerceptron(nf, 16), lin1=torch.nn.Linear(nf, 256), lin2=torch.nn.Linear(256, int(c['n_classes']))))
    assert sum(p.numel() for p in mods.parameters()) == int(c['n_params'])
    mods = fill_params(mods)
    head = LinearCrossEntropy(256, int(c['n_classes']))
    head.load_state_dict(mods['lin2'].state_dict())          # the fixture's lin2.* (param_fill on both sides)
    mods['lin2'] = head
    mods = mods.to(dev)

    class Mesh:
        pass
    d = Mesh()
    d.logMag, d.logAng, d.w, d.supp_edges, d.xp = (D(c[k], dev) for k in ('logMag', 'logAng', 'w', 'edges', 'xp'))
    edges, sten, ln, wxp = FCPrecomp(B, R, float(c['eps']))(d)
    conv = (edges, sten)
    x1 = mods['lift'](D(c['pos'], dev), edges, sten[..., B:B + 2])
    x = mods['resnet1'](x1, *conv)
    x2 = mods['resnet2'](x, *conv) + mods['res1'](x1)
    x = mods['resnet3'](x2, *conv)
    x3 = mods['resnet4'](x, *conv) + mods['res2'](x2)
    x = mods['resnet5'](x3, *conv)
    x4 = mods['resnet6'](x, *conv) + mods['res3'](x3)
    x = mods['resnet7'](x4, *conv)
    x = mods['resnet8'](x, *conv) + mods['res4'](x4)
    h = mods['echo'](x, edges, sten, ln, wxp)
    loss = mods['lin2'](torch.relu(mods['lin1'](h)), D(c['labels'], dev))
    print('loss %.7f, recorded %.7f' % (float(loss.detach()), float(c['loss'])))
    assert abs(float(loss.detach()) - float(c['loss'])) < 1e-4 * max(1.0, abs(float(c['loss'])))
    params = dict(mods.named_parameters())
    grads = torch.autograd.grad(loss, list(params.values()))
    report = []
    for (name, _), g in zip(params.items(), grads):
        sub, stats = grad_sample(Hn(g))
        e = rel_err(sub, c['g_' + name])
        cond = float(c['gcond_' + name])
        report.append((e / max(cond, 5e-6), e, cond, name))
        assert abs(stats[0] - c['gstat_' + name][0]) < 0.05 * c['gstat_' + name][0] + 1e-12, name
    report.sort(reverse=True)
    print('gradient samples, worst by (error / perturbed-twin deviation): ' + ', '.join('%s %.1e / %.1e' % (n, e, cd) for _, e, cd, n in report[:5]))
    for ratio, e, cond, name in report:
        assert e < max(2e-5, 4 * cond), (name, e, cond)
