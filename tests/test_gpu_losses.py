"""TwinLoss, TwinEval, LabelSmoothingLoss and the pair kernels under them (csrc/fc_loss.hip) on the device: parity with the
reference's fixtures (tests/golden/losses.npz) at the project's gates -- rel_err <= 1e-5 in float32, 1e-12 in float64 -- exact
agreement of the pair distance and of the dense counts with the numpy restatement, the complement forms against explicit
lists, StepGraph replay, guard bands around every buffer, and a training step through a convolution block."""
import numpy as np
import pytest
import torch

import _losses_ref as ref
from conftest import load_golden, rel_err

pytestmark = pytest.mark.gpu

F32_GATE = 1e-5
F64_GATE = 1e-12


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return t.to(dev) if dtype is None else t.to(device=dev, dtype=dtype)


def N_(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------ parity with the reference's fixtures
@pytest.mark.parametrize('tag', ['f32', 'f64'])
@pytest.mark.parametrize('name', ['twin_n300', 'twin_repeat'])
def test_twin_loss_matches_reference(dev, name, tag):
    """Value and both gradients against the reference's TwinLoss run with the same yN.  'twin_repeat': every pair hits row 5 of xT
    and one of a few rows of xS.  The reference returns a float32 loss whatever the features' dtype (it accumulates into
    torch.empty(1).float()); we return the features' dtype.  In float64 the fixture's loss therefore carries float32's rounding:
    ours is held to 1e-12 against the float64 restatement (which tests/test_losses_host.py ties to the fixture bit for bit after
    the reference's own two roundings) and to two float32 roundings, 2 * 2^-24, against the fixture itself."""
    from fieldconv_amd.losses import twin_loss
    c = load_golden('losses.npz')[name]
    dt = torch.float32 if tag == 'f32' else torch.float64
    gate = F32_GATE if tag == 'f32' else F64_GATE
    xS = T(c['xS'], dev, dt).requires_grad_(True)
    xT = T(c['xT'], dev, dt).requires_grad_(True)
    loss = twin_loss(xS, xT, T(c['p'], dev), T(c['n'], dev), T(c['yN'], dev), float(c['mu']))
    assert tuple(loss.shape) == (1,) and loss.dtype == dt
    gS, gT = torch.autograd.grad(loss, [xS, xT])
    errs = dict(loss=rel_err(N_(loss), c[f'loss_{tag}'].astype(np.float64)), gS=rel_err(N_(gS), c[f'gS_{tag}']), gT=rel_err(N_(gT), c[f'gT_{tag}']))
    lp, ln, _, _ = ref.twin_loss(c['xS'], c['xT'], c['p'], c['n'], c['yN'], float(c['mu']))
    errs['loss_vs_restatement'] = rel_err(N_(loss).astype(np.float64), np.array([lp + ln]))
    print(name, tag, errs)
    assert errs['gS'] <= gate and errs['gT'] <= gate
    assert errs['loss_vs_restatement'] <= gate
    assert errs['loss'] <= (gate if tag == 'f32' else 2.0 ** -23)
    # rows no pair touches have exactly zero gradient
    untouched = np.setdiff1d(np.arange(c['xT'].shape[0]), np.concatenate((c['p'][:, 0], c['n'][:, 0])))
    assert untouched.size and not N_(gT)[untouched].any()


@pytest.mark.parametrize('shape', ['ls_1024x8', 'ls_1x30', 'ls_257x40'])
def test_label_smoothing_matches_reference(dev, shape):
    from fieldconv_amd.nn import LabelSmoothingLoss
    c = load_golden('losses.npz')[shape]
    for v in c['variants']:
        smoothing, weighted, classes, ndt = ref.parse_variant(str(v))
        dt = torch.float32 if ndt == np.float32 else torch.float64
        gate = F32_GATE if ndt == np.float32 else F64_GATE
        pred = T(c['pred'], dev, dt).requires_grad_(True)
        weight = T(c['weight'], dev, dt) if weighted else None
        loss = LabelSmoothingLoss(classes, smoothing=smoothing, dim=1, weight=weight)(pred, T(c['target'], dev))
        assert loss.dim() == 0 and loss.dtype == dt
        gp, = torch.autograd.grad(loss, [pred])
        e_loss, e_grad = rel_err(N_(loss), c[f'loss_{v}']), rel_err(N_(gp), c[f'gpred_{v}'])
        print(shape, v, e_loss, e_grad)
        assert e_loss <= gate and e_grad <= gate, (shape, v)
    # an upstream gradient other than 1 scales the gradient
    pred = T(c['pred'], dev, torch.float64).requires_grad_(True)
    loss = LabelSmoothingLoss(c['pred'].shape[1], smoothing=0.1)(pred, T(c['target'], dev))
    g1, = torch.autograd.grad(loss, [pred], retain_graph=True)
    g3, = torch.autograd.grad(3.0 * loss, [pred])
    assert rel_err(N_(g3), 3.0 * N_(g1)) <= 1e-15


def test_twin_eval_matches_reference_counts(dev):
    from fieldconv_amd.nn import TwinEval
    for name, c in load_golden('losses.npz').items():
        if not name.startswith('twin_'):
            continue
        for tag, dt in (('f32', torch.float32), ('f64', torch.float64)):
            out = TwinEval(mu=float(c['mu']), ratio=float(c['eval_ratio']))(T(c['xS'], dev, dt), T(c['xT'], dev, dt), T(c['p'], dev), T(c['n'], dev))
            assert out == (int(c[f'nFN_{tag}']), int(c[f'nFP_{tag}'])) and all(type(v) is int for v in out)


# ------------------------------------------------------------------ exactness against the numpy restatement
DENSE_SHAPES = [(2048, 2048, 16), (1000, 777, 16), (65, 4099, 3), (300, 300, 48)]


def _features(n_T, n_S, C, seed):
    rng = np.random.default_rng(seed)
    return (0.9 * rng.random((n_S, C))).astype(np.float32), (0.9 * rng.random((n_T, C))).astype(np.float32)


def _thresholds(D, n):
    """n thresholds: inside the data's range (quantiles, and one exactly equal to a distance that occurs) and outside it on
    both sides"""
    if n == 1:
        return [float(np.median(D))]
    inside = [float(q) for q in np.quantile(D, np.linspace(0.02, 0.98, n - 4))]
    return [0.0, float(D.min()) * 0.5, float(D.flat[12345 % D.size])] + inside + [float(D.max()) * 2.0]


@pytest.mark.parametrize('n_T,n_S,C', DENSE_SHAPES)
def test_pair_sqdist_is_bit_exact(dev, n_T, n_S, C):
    from fieldconv_amd.losses import pair_sqdist
    xS, xT = _features(n_T, n_S, C, seed=n_T + C)
    rng = np.random.default_rng(1)
    pairs = np.stack((rng.integers(0, n_T, 5000), rng.integers(0, n_S, 5000)), 1)
    pairs[:3] = [[0, 0], [n_T - 1, n_S - 1], [n_T - 1, 0]]
    for ndt, dt in ((np.float32, torch.float32), (np.float64, torch.float64)):
        got = pair_sqdist(T(xS, dev, dt), T(xT, dev, dt), T(pairs, dev))
        want = ref.sqdist(xT.astype(ndt)[pairs[:, 0]], xS.astype(ndt)[pairs[:, 1]])
        assert got.dtype == dt and np.array_equal(N_(got).view(np.uint32 if ndt == np.float32 else np.uint64),
                                                  want.view(np.uint32 if ndt == np.float32 else np.uint64))
    for bad in ([n_T, 0], [0, n_S], [-1, 0]):
        with pytest.raises(IndexError):
            pair_sqdist(T(xS, dev), T(xT, dev), T(np.array([[0, 0], bad]), dev))
    with pytest.raises(ValueError):
        pair_sqdist(T(xS, dev), T(xT[:, :-1] if C > 1 else xT, dev, torch.float64), T(pairs, dev))


@pytest.mark.parametrize('n_thr', [1, 16])
@pytest.mark.parametrize('n_T,n_S,C', DENSE_SHAPES)
def test_dense_counts_are_exact(dev, n_T, n_S, C, n_thr):
    """fc_twin_count_dense and twin_eval_curve against counts taken from the float32 restatement of every pair."""
    from fieldconv_amd.losses import twin_count_dense
    from fieldconv_amd.utils import twin_eval_curve
    xS, xT = _features(n_T, n_S, C, seed=n_T + C)
    D = ref.dense_sqdist(xT, xS)
    thr = _thresholds(D, n_thr)
    thr32 = np.array(thr, dtype=np.float32)
    below, above = twin_count_dense(T(xS, dev), T(xT, dev), thr)
    assert below.dtype == torch.int64 and tuple(below.shape) == (n_thr,)
    want_below = np.array([(D < t).sum() for t in thr32]), np.array([(D > t).sum() for t in thr32])
    assert np.array_equal(N_(below), want_below[0]) and np.array_equal(N_(above), want_below[1])
    if n_thr > 1:
        assert want_below[0][0] == 0 and want_below[0][-1] == D.size and want_below[1][-1] == 0          # outside the range, both ways
        assert (below + above)[2].item() < D.size                                                        # a threshold some pair sits on
    # the curve: positives as listed (with duplicates), false positives over the complement of the distinct positives
    rng = np.random.default_rng(2)
    P = min(n_T, n_S)
    pos = np.stack((rng.permutation(n_T)[:P], rng.integers(0, n_S, P)), 1)
    pos = np.concatenate((pos, pos[:P // 4]))
    n_fn, n_fp = twin_eval_curve(T(xS, dev), T(xT, dev), T(pos, dev), thr)
    dpos = D[pos[:, 0], pos[:, 1]]
    mask = np.ones(D.shape, dtype=bool)
    mask[pos[:, 0], pos[:, 1]] = False
    assert np.array_equal(N_(n_fn), np.array([(dpos > t).sum() for t in thr32]))
    assert np.array_equal(N_(n_fp), np.array([(D[mask] < t).sum() for t in thr32]))
    # float64 features: the same counts from the float64 restatement (one threshold set, smaller cases)
    if n_T * n_S <= 10 ** 6:
        D64 = ref.dense_sqdist(xT.astype(np.float64), xS.astype(np.float64))
        b64, a64 = twin_count_dense(T(xS, dev, torch.float64), T(xT, dev, torch.float64), thr)
        assert np.array_equal(N_(b64), np.array([(D64 < t).sum() for t in thr])) and np.array_equal(N_(a64), np.array([(D64 > t).sum() for t in thr]))


def test_counts_against_the_reference_formula_2048(dev):
    """The reference's TwinEval sums (xT[a] - xS[b])^2 in torch's own order, so its float32 d2 is not ours bit for bit.  Each is
    a sum of C non-negative float32 terms with relative error below (C + 1) 2^-24, so the two counts can differ only by pairs
    whose exact d2 lies within (C + 2) 2^-23 thr of thr.  The input keeps that band below 0.01 % of the pairs."""
    from fieldconv_amd.losses import twin_count_dense
    N, C, thr = 2048, 16, 2.5
    torch.manual_seed(1)
    xS, xT = 0.9 * torch.rand(N, C), 0.9 * torch.rand(N, C)
    D64 = ((xT.double()[:, None, :] - xS.double()[None, :, :]) ** 2).sum(-1)
    band = int(((D64 - thr).abs() <= (C + 2) * 2.0 ** -23 * thr).sum())
    # the reference's formula, on the CPU, over all pairs (row blocks of the broadcast difference)
    ref_below = sum(int((torch.sum(torch.pow(xT[a:a + 256, None, :] - xS[None, :, :], 2), dim=2) < thr).sum()) for a in range(0, N, 256))
    below, above = twin_count_dense(xS.to(dev), xT.to(dev), [thr])
    print('band', band, 'reference count', ref_below, 'ours', int(below), 'exact', int((D64 < thr).sum()))
    assert band < 1e-4 * N * N and 0.25 * N * N < ref_below < 0.75 * N * N
    assert abs(int(below) - ref_below) <= band
    assert int(below) + int(above) + int((T(ref.dense_sqdist(xT.numpy(), xS.numpy()), dev) == thr).sum()) == N * N


# ------------------------------------------------------------------ modules against the functional forms
def test_twin_eval_complement_equals_explicit_list(dev):
    from fieldconv_amd.nn import TwinEval
    from fieldconv_amd.utils import null_pair_count, null_pairs_from_rank
    n_T, n_S, C = 300, 257, 16
    xS, xT = _features(n_T, n_S, C, seed=3)
    rng = np.random.default_rng(3)
    pos = np.stack((rng.integers(0, n_T, 400), rng.integers(0, n_S, 400)), 1)
    pos = np.concatenate((pos, pos[:50]))
    p_ = T(pos, dev)
    count = null_pair_count(p_, n_T, n_S)
    n_ = null_pairs_from_rank(p_, n_T, n_S, torch.arange(count, device=dev))
    want = np.setdiff1d(np.arange(n_T * n_S), pos[:, 0] * n_S + pos[:, 1])
    assert np.array_equal(N_(n_[:, 0] * n_S + n_[:, 1]), want)
    for mu in (5, 4.2, 8):
        ev = TwinEval(mu=mu)
        assert ev(T(xS, dev), T(xT, dev), p_, None) == ev(T(xS, dev), T(xT, dev), p_, n_) == ev(T(xS, dev), T(xT, dev), p_)
    D = ref.dense_sqdist(xT, xS)
    nFN, nFP = TwinEval()(T(xS, dev), T(xT, dev), p_, None)
    assert nFN == int((D[pos[:, 0], pos[:, 1]] > np.float32(2.5)).sum()) and nFP == int((D.ravel()[want] < np.float32(2.5)).sum()) and nFP > 0
    with pytest.raises(IndexError):
        TwinEval()(T(xS, dev), T(xT, dev), T(np.array([[0, n_S]]), dev), None)


def test_twin_loss_module_draws_its_weights_from_torchs_generator(dev):
    from fieldconv_amd.losses import twin_loss
    from fieldconv_amd.nn import TwinLoss
    from fieldconv_amd.utils import sample_null_pairs
    n_T, n_S, C = 500, 400, 16
    xS, xT = (T(a, dev) for a in _features(n_T, n_S, C, seed=4))
    p_ = torch.stack((torch.arange(300, device=dev), torch.arange(300, device=dev) % n_S), 1)
    n_ = sample_null_pairs(p_, n_T, n_S, 512)
    torch.manual_seed(9)
    a = TwinLoss()(xS, xT, p_, n_)
    torch.manual_seed(9)
    yN = 0.2 * torch.rand(512, device=dev).float()
    assert torch.equal(a, twin_loss(xS, xT, p_, n_, yN, 5))
    assert not torch.equal(a, TwinLoss()(xS, xT, p_, n_))          # the next draw differs


@pytest.mark.parametrize('tag', ['f32', 'f64'])
def test_twin_loss_is_bitwise_reproducible(dev, tag):
    """Forward + backward twice on the repeated-row fixture and on a list long enough for several workgroups."""
    from fieldconv_amd.losses import twin_loss
    dt = torch.float32 if tag == 'f32' else torch.float64
    c = load_golden('losses.npz')['twin_repeat']
    rng = np.random.default_rng(5)
    big_S, big_T = _features(700, 900, 24, seed=5)
    cases = [(c['xS'], c['xT'], c['p'], c['n'], c['yN'], 2.5),
             (big_S, big_T, np.stack((rng.integers(0, 700, 3000), rng.integers(0, 900, 3000)), 1),
              np.stack((rng.integers(0, 700, 2500) % 7, rng.integers(0, 900, 2500)), 1), (0.2 * rng.random(2500)).astype(np.float32), 3.0)]
    for xS, xT, p, n, yN, mu in cases:
        runs = []
        for _ in range(2):
            a, b = T(xS, dev, dt).requires_grad_(True), T(xT, dev, dt).requires_grad_(True)
            loss = twin_loss(a, b, T(p, dev), T(n, dev), T(yN, dev), mu)
            runs.append((loss.detach(),) + torch.autograd.grad(loss, [a, b]))
        assert all(torch.equal(u, v) for u, v in zip(*runs))
        lp, ln, gS, gT = ref.twin_loss(xS, xT, p, n, yN, mu)
        gate = F32_GATE if tag == 'f32' else F64_GATE
        assert rel_err(N_(runs[0][0]).astype(np.float64), np.array([lp + ln])) <= gate
        assert rel_err(N_(runs[0][1]), gS) <= gate and rel_err(N_(runs[0][2]), gT) <= gate


def test_out_of_range_pair_in_twin_loss_gives_nan_not_a_fault(dev):
    from fieldconv_amd.losses import twin_loss
    xS, xT = (T(a, dev).requires_grad_(True) for a in _features(40, 30, 16, seed=6))
    p_ = T(np.array([[0, 0], [39, 29]]), dev)
    n_ = T(np.array([[1, 1], [40, 0], [2, 2]]), dev)
    loss = twin_loss(xS, xT, p_, n_, torch.full((3,), 0.1, device=dev), 5)
    gS, gT = torch.autograd.grad(loss, [xS, xT])
    assert torch.isnan(loss).all() and torch.isnan(gS[0]).all() and torch.isfinite(gT[39]).all()


# ------------------------------------------------------------------ StepGraph
def test_losses_replay_in_a_step_graph(dev):
    from fieldconv_amd.losses import twin_loss
    from fieldconv_amd.nn import LabelSmoothingLoss, TwinLoss
    from fieldconv_amd.utils import StepGraph
    c = load_golden('losses.npz')['twin_n300']
    xS, xT = T(c['xS'], dev).requires_grad_(True), T(c['xT'], dev).requires_grad_(True)
    p_, n_, yN = T(c['p'], dev), T(c['n'], dev), T(c['yN'], dev)

    def twin_step():
        loss = twin_loss(xS, xT, p_, n_, yN, 2.5)
        return (loss.detach(),) + torch.autograd.grad(loss, [xS, xT])
    eager = [t.clone() for t in twin_step()]
    graphed = StepGraph(twin_step)
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(eager, graphed.replay()))
    with torch.no_grad():
        xS.mul_(1.05)
    replayed = [t.clone() for t in graphed.replay()]
    assert all(torch.equal(a, b) for a, b in zip(twin_step(), replayed)) and not torch.equal(replayed[0], eager[0])

    # the module draws yN inside the captured step: every replay redraws, so only capturability and finiteness are checked
    module = TwinLoss(mu=2.5)

    def module_step():
        loss = module(xS, xT, p_, n_)
        return (loss.detach(),) + torch.autograd.grad(loss, [xS, xT])
    g2 = StepGraph(module_step)
    first = [t.clone() for t in g2.replay()]
    second = g2.replay()
    assert all(torch.isfinite(t).all() for t in first) and not torch.equal(first[0], second[0])

    ls = load_golden('losses.npz')['ls_257x40']
    pred = T(ls['pred'], dev).requires_grad_(True)
    target, weight = T(ls['target'], dev), T(ls['weight'], dev)
    crit = LabelSmoothingLoss(40, smoothing=0.1, dim=1, weight=weight)

    def ls_step():
        loss = crit(pred, target)
        return (loss.detach(),) + torch.autograd.grad(loss, [pred])
    eager = [t.clone() for t in ls_step()]
    g3 = StepGraph(ls_step)
    for _ in range(2):
        assert all(torch.equal(a, b) for a, b in zip(eager, g3.replay()))


# ------------------------------------------------------------------ guard bands (in the style of tests/test_gpu_canary.py)
GUARD = 4096
PATTERN = 0xA5


class _GuardedTorch:
    """Stands in for `torch` inside fieldconv_amd.losses: device `empty` returns a view into an allocation with GUARD bytes of
    PATTERN on both sides."""

    def __init__(self):
        self.blocks = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *size, dtype=None, device=None, **kw):
        if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
            size = tuple(size[0])
        if device is None or torch.device(device).type != 'cuda' or kw:
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        dtype = dtype or torch.float32
        n = int(np.prod(size)) if len(size) else 1
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=device)
        self.blocks.append((buf, nbytes))
        if nbytes == 0:
            return torch.empty(size, dtype=dtype, device=device)
        return buf[GUARD:GUARD + nbytes].view(dtype).view(tuple(size))

    def check(self, what):
        torch.cuda.synchronize()
        bad = [(i, nbytes) for i, (buf, nbytes) in enumerate(self.blocks)
               if not bool((buf[:GUARD] == PATTERN).all()) or not bool((buf[GUARD + nbytes:] == PATTERN).all())]
        assert not bad, f'{what}: writes outside a buffer (allocation index, payload bytes): {bad}'
        n = len(self.blocks)
        self.blocks = []
        return n


@pytest.mark.parametrize('n_T,n_S,C,P,M', [(300, 257, 16, 200, 256), (65, 4099, 3, 1500, 1100), (129, 70, 48, 64, 2000), (1, 1, 1, 1, 1)])
def test_no_write_outside_any_buffer(dev, monkeypatch, n_T, n_S, C, P, M):
    """Every output, saved buffer and workspace of the loss entry points is carved out of a larger allocation whose margins hold a
    byte pattern; after forward + backward of each family the margins are untouched."""
    from fieldconv_amd import _launch, losses
    g = _GuardedTorch()
    monkeypatch.setattr(losses, 'torch', g)
    monkeypatch.setattr(_launch, 'torch', g)
    rng = np.random.default_rng(P)
    xS_np, xT_np = _features(n_T, n_S, C, seed=7)
    pos = T(np.stack((rng.integers(0, n_T, P), rng.integers(0, n_S, P)), 1), dev)
    neg = T(np.stack((rng.integers(0, n_T, M), rng.integers(0, n_S, M)), 1), dev)
    n = 0
    for dt in (torch.float32, torch.float64):
        xS, xT = T(xS_np, dev, dt).requires_grad_(True), T(xT_np, dev, dt).requires_grad_(True)
        loss = losses.twin_loss(xS, xT, pos, neg, T((0.2 * rng.random(M)).astype(np.float32), dev), 2.5)
        torch.autograd.grad(loss, [xS, xT])
        n += g.check('twin_loss')
        losses.pair_sqdist(xS, xT, neg)
        losses.twin_count_dense(xS, xT, [2.0])
        losses.twin_count_dense(xS, xT, [0.5 * k for k in range(16)])
        losses.twin_eval(xS, xT, pos, None, 2.5)
        n += g.check('pair_sqdist / twin_count_dense / twin_eval')
        for K in (C, 40):
            pred = torch.randn(n_T, K, device=dev, dtype=dt, requires_grad=True)
            loss = losses.label_smoothing_loss(pred, torch.randint(0, K, (n_T,), device=dev), K + 1, 0.1, torch.rand(K, device=dev, dtype=dt))
            torch.autograd.grad(loss, [pred])
        n += g.check('label_smoothing_loss')
    assert n >= 2 * (5 + 5 + 6)


# ------------------------------------------------------------------ end to end
def test_feature_matching_step_reaches_the_convolution(dev):
    """Descriptors softAbs(TangentPerceptron(FCResNetBlock(x))) of two feature fields on one sphere sampling, sampled negatives,
    TwinLoss, backward: the block's parameters get finite non-zero gradients, equal within the float32 gate to those of the same
    step with the loss written in stock torch ops."""
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.losses import twin_loss
    from fieldconv_amd.nn import FCResNetBlock, TangentPerceptron, TwinLoss
    from fieldconv_amd.utils import sample_null_pairs, softAbs
    from oracle.torch_composites import FCPrecomp           # the tests build their stencils on the CPU
    N, k, C, D, B, R = 300, 24, 16, 16, 2, 6
    data = sphere_support(N, k).to(dev)
    edges, sten, _, _ = FCPrecomp(B, R, data.epsilon)(data)
    torch.manual_seed(11)
    block = FCResNetBlock(C, C, band_limit=B, n_rings=R).to(dev)
    head = TangentPerceptron(C, D).to(dev)
    params = list(block.parameters()) + list(head.parameters())
    fS = torch.complex(torch.randn(N, C), torch.randn(N, C)).to(dev)
    fT = torch.complex(torch.randn(N, C), torch.randn(N, C)).to(dev)
    pos = torch.stack((torch.arange(N, device=dev), torch.randperm(N).to(dev)), 1)[:200]
    neg = sample_null_pairs(pos, N, N, 256)
    mu = 5

    def descriptors():
        return softAbs(head(block(fS, edges, sten))), softAbs(head(block(fT, edges, sten)))

    xS, xT = descriptors()
    assert xS.dtype == torch.float32 and tuple(xS.shape) == (N, D)
    torch.manual_seed(21)
    loss = TwinLoss(mu=mu)(xS, xT, pos, neg)
    grads = torch.autograd.grad(loss, params)
    torch.manual_seed(21)
    yN = 0.2 * torch.rand(256, device=dev).float()
    xS2, xT2 = descriptors()
    dP = torch.sum(torch.pow(xT2[pos[:, 0], :] - xS2[pos[:, 1], :], 2), dim=1)
    dN = torch.sum(torch.pow(xT2[neg[:, 0], :] - xS2[neg[:, 1], :], 2), dim=1)
    stock = dP.sum() / 200 + (torch.sum(dN * yN) + torch.sum(torch.relu(mu - dN) * (1 - yN))) / 256
    grads2 = torch.autograd.grad(stock, params)
    print('loss', float(loss.detach()), 'stock', float(stock.detach()))
    assert rel_err(N_(loss), N_(stock).reshape(1)) <= F32_GATE
    # The gate is on the step's whole gradient (max |difference| over max |reference|, as everywhere), and on each parameter whose
    # gradient is a sizeable part of it.  Not on every parameter alone: the descriptors are moduli, so a parameter that only turns a
    # channel's phase has an exactly zero gradient, and both computations return rounding noise (1e-8) for it.
    ga = [N_(torch.view_as_real(t) if t.is_complex() else t) for t in grads]
    gb = [N_(torch.view_as_real(t) if t.is_complex() else t) for t in grads2]
    assert all(np.isfinite(a).all() and np.abs(a).max() > 0 for a in ga)
    whole = np.abs(np.concatenate([b.ravel() for b in gb])).max()
    assert max(np.abs(a - b).max() for a, b in zip(ga, gb)) <= F32_GATE * whole
    sizeable = [(p, a, b) for p, a, b in zip(params, ga, gb) if np.abs(b).max() >= 0.01 * whole]
    assert any(p is q for q in block.parameters() for p, _, _ in sizeable)          # the convolution block is among them
    for p, a, b in sizeable:
        assert rel_err(a, b) <= F32_GATE, tuple(p.shape)
    assert torch.equal(loss, twin_loss(xS, xT, pos, neg, yN, mu))
