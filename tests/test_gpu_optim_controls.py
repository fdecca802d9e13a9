"""fc_adam_step_ctl (csrc/fc_optim.hip) and the controls of fieldconv_amd.optim.FusedAdam: device learning rate, global-norm clipping,
the skip of a non-finite gradient, decoupled weight decay and the moving average.

The entry point is called directly on flat buffers and compared against the numpy restatement of its formulas
(tests/_optim_controls_ref.py, pinned to torch on the CPU by tests/test_optim_controls_host.py): float64 is the reference, float32
in the kernel's order of operations is the restatement whose own error, times 4 with a floor of 1e-6, is the gate (_optim_ref.gate_of,
the gate of tests/test_gpu_optim.py).  Parameters are measured against max(|their change|, one ulp), as there.

Sizes: _optim_ref.SIZES and two that follow from the kernel's constants (csrc/fc_optim.hip): a workgroup of the sum of squares covers
CHUNK = 256 threads x 4 float4 = 4096 floats, and the finalize workgroup has 256 threads."""
import functools

import numpy as np
import pytest
import torch

import _optim_controls_ref as cref
import _optim_ref as oref

pytestmark = pytest.mark.gpu
FC_OK = 0
CHUNK, FINALIZE_THREADS = 4096, 256
N_PAST_TWO = 2 * CHUNK + 4                          # one float4 past two whole workgroups of the sum of squares: 3 partials
N_MANY = (FINALIZE_THREADS + 1) * CHUNK + 4         # 258 partials: more than the finalize workgroup has threads (n < 2^22)
SIZES = oref.SIZES + (N_PAST_TWO, N_MANY)
LR = oref.HYPER['lr']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def inputs(n, t):
    """_optim_ref.inputs, computed once per (n, t) and left unchanged (read-only arrays)"""
    out = oref.inputs(n, t)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def norm_of(n, t):
    return cref.grad_norm(inputs(n, t)[0])


def parts_of(n):
    return (n + CHUNK - 1) // CHUNK


class Buffers:
    """device copies of (p, g, m, v[, ema]), the step counter, the rate and the statistics for fc_adam_step_ctl"""

    def __init__(self, dev, p, g, m, v, step_before, ema=None, lr=LR, n_skipped=0.0):
        from fieldconv_amd import _lib
        self.lib, self.dev = _lib.load(), dev
        up = lambda a: None if a is None else torch.from_numpy(np.array(a, np.float32)).to(dev)      # noqa: E731
        self.p, self.g, self.m, self.v, self.ema = (up(a) for a in (p, g, m, v, ema))
        self.step = torch.full((1,), float(step_before), dtype=torch.float32, device=dev)
        self.lr = torch.full((1,), lr, dtype=torch.float32, device=dev)
        self.stats = torch.tensor([-1.0, -1.0, -1.0, n_skipped], dtype=torch.float32, device=dev)
        self.ws = torch.empty(self.lib.fc_adam_ctl_workspace_bytes(max(self.p.numel(), 4)), dtype=torch.uint8, device=dev)

    def call(self, n=None, weight_decay=0.0, decoupled=False, max_norm=0.0, skip_nonfinite=False, ema_decay=None):
        from fieldconv_amd import _lib
        from fieldconv_amd._launch import _p, _po, stream
        h = oref.HYPER
        ctl = _lib.FcAdamCtl(h['beta1'], h['beta2'], h['eps'], weight_decay, int(decoupled), max_norm, int(skip_nonfinite),
                             -1.0 if ema_decay is None else ema_decay)
        n = self.p.numel() if n is None else n
        status = self.lib.fc_adam_step_ctl(_p(self.p), _p(self.g), _p(self.m), _p(self.v), _po(self.ema), _p(self.step), _p(self.lr),
                                           _p(self.stats), _p(self.ws), self.ws.numel(), n, ctl, stream())
        torch.cuda.synchronize()
        return status

    def host(self):
        out = {k: H(getattr(self, k)) for k in ('p', 'g', 'm', 'v', 'stats')}
        out['ema'] = None if self.ema is None else H(self.ema)
        out['t'] = float(self.step.item())
        return out


def old_step(dev, p, g, m, v, step_before, n, weight_decay):
    """fc_adam_step on copies of the buffers -> (p, m, v, counter)"""
    from fieldconv_amd import _lib
    from fieldconv_amd._launch import _p, stream
    t = [torch.from_numpy(np.array(a, np.float32)).to(dev) for a in (p, g, m, v)]
    step = torch.full((1,), float(step_before), dtype=torch.float32, device=dev)
    h = oref.HYPER
    assert _lib.load().fc_adam_step(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(step), n, h['lr'], h['beta1'], h['beta2'], h['eps'],
                                    weight_decay, stream()) == FC_OK
    torch.cuda.synchronize()
    return H(t[0]), H(t[2]), H(t[3]), float(step.item())


def assert_within_gate(got, want, own, p_before, label):
    """p against max(|change|, ulp), m, v and ema relatively; the gate from the float32 restatement's own error -> the figures"""
    line = []
    for k in ('p', 'm', 'v', 'ema'):
        if want[k] is None:
            continue
        if k == 'p':
            fl = cref.p_floor(p_before, want['p'])
            err, own_err = cref.floor_err(got['p'], want['p'], fl), cref.floor_err(own['p'], want['p'], fl)
        else:
            err, own_err = oref.rel_err(got[k], want[k]), oref.rel_err(own[k], want[k])
        line.append('%s %.2e (own %.2e, gate %.2e)' % (k, err, own_err, oref.gate_of(own_err)))
        assert err <= oref.gate_of(own_err), (label, k, line)
    print('\n%s: %s' % (label, '  '.join(line)))


# ------------------------------------------------------------------------------------------------ 1. neutral == fc_adam_step
@pytest.mark.parametrize('t', oref.STEPS)
@pytest.mark.parametrize('n', SIZES)
def test_neutral_controls_give_the_old_bits(n, t, dev):
    g, m, v, p0, _ = inputs(n, t)
    for wd in (0.0, 1e-2):
        b = Buffers(dev, p0, g, m, v, t - 1, n_skipped=3.0)
        assert b.call(weight_decay=wd) == FC_OK
        got = b.host()
        p1, m1, v1, counter = old_step(dev, p0, g, m, v, t - 1, n, wd)
        assert got['t'] == counter == float(t)
        assert same_bits(got['p'], p1) and same_bits(got['m'], m1) and same_bits(got['v'], v1)
        assert not same_bits(got['p'], p0) and same_bits(got['g'], g)
        assert got['stats'].tolist() == [0.0, 1.0, 0.0, 3.0]             # nothing wanted: the finalize launch only ticks


# ------------------------------------------------------------------------------------------------ 2. the norm
@pytest.mark.parametrize('n', SIZES)
def test_norm_is_the_rounded_exact_norm(n, dev):
    """|stats[0] - float32(norm by fsum)| <= 1 float32 ulp: the double sum of n <= 2^22 exact squares is off by at most 2^22 2^-53
    relatively, far below half a float32 ulp, so only the final rounding can differ (double rounding)."""
    g, m, v, p0, _ = inputs(n, 1)
    runs = []
    for _ in range(2):
        b = Buffers(dev, p0, g, m, v, 0)
        assert b.call(skip_nonfinite=True) == FC_OK
        runs.append(b.host())
    got = runs[0]['stats']
    print('\nnorm n=%d: device %.9g  fsum %.9g  ulps %d' % (n, got[0], np.float32(norm_of(n, 1)), cref.ulps(got[0], norm_of(n, 1))))
    assert cref.ulps(got[0], norm_of(n, 1)) <= 1 and got[1:].tolist() == [1.0, 0.0, 0.0]
    assert all(same_bits(runs[0][k], runs[1][k]) for k in ('stats', 'p', 'm', 'v'))                # two runs, the same bits
    # the tail zeroed from a 16-byte boundary on: the norm of the shorter vector -- and the bits of a call on the shorter vector,
    # since the zeros enter the same additions exactly
    if n >= 8:
        k = (n // 2 + 3) // 4 * 4 if n < 2 * CHUNK else n - CHUNK - 8              # (large sizes: the cut inside the last but one workgroup)
        short = np.array(g)
        short[k:] = 0
        want = cref.grad_norm(short[:k])
        b = Buffers(dev, p0, short, m, v, 0)
        assert b.call(skip_nonfinite=True) == FC_OK
        zeroed = b.host()['stats']
        b = Buffers(dev, p0, g, m, v, 0)
        assert b.call(n=k, skip_nonfinite=True) == FC_OK
        shorter = b.host()['stats']
        assert cref.ulps(zeroed[0], want) <= 1 and same_bits(zeroed, shorter)


# ------------------------------------------------------------------------------------------------ 3. clipping
@pytest.mark.parametrize('factor', [0.5, 1.0, 2.0])
@pytest.mark.parametrize('n', SIZES)
def test_clipping(n, factor, dev):
    """max_norm at 0.5 x, 1 x and 2 x the norm.  The coefficient against the restatement's (the double formula on the fsum norm, rounded
    once): 1 ulp, since the device's double norm may differ from fsum's in its last place; p, m, v against the float64 restatement fed
    the device's own coefficient, so that the update is gated on its own."""
    t, wd = 2, 1e-2
    g, m, v, p0, _ = inputs(n, t)
    max_norm = float(np.float32(factor * norm_of(n, t)))
    b = Buffers(dev, p0, g, m, v, t - 1)
    assert b.call(weight_decay=wd, max_norm=max_norm) == FC_OK
    got = b.host()
    coef = got['stats'][1]
    want_coef = cref.clip_coef(norm_of(n, t), max_norm)
    print('\nclip n=%d x%.1f: coef %.9g  restatement %.9g' % (n, factor, coef, want_coef))
    assert cref.ulps(coef, want_coef) <= 1 and cref.ulps(got['stats'][0], norm_of(n, t)) <= 1
    assert got['stats'][2:].tolist() == [0.0, 0.0] and got['t'] == float(t)
    assert (factor, bool(coef < 1)) in ((0.5, True), (1.0, True), (1.0, False), (2.0, False))
    kw = dict(weight_decay=wd, max_norm=max_norm, coef=coef)
    want = cref.step_ctl(p0, g, m, v, None, t - 1, LR, np.float64, **kw)
    own = cref.step_ctl(p0, g, m, v, None, t - 1, LR, np.float32, **kw)
    assert_within_gate(got, want, own, p0, 'clip n=%d x%.1f' % (n, factor))
    assert same_bits(got['g'], g)                                            # the gradient buffer is not rewritten
    if coef == 1:                                                            # no clipping: the unclipped bits
        p1, m1, v1, _ = old_step(dev, p0, g, m, v, t - 1, n, wd)
        assert same_bits(got['p'], p1) and same_bits(got['m'], m1) and same_bits(got['v'], v1)
    else:
        assert not same_bits(got['m'], old_step(dev, p0, g, m, v, t - 1, n, wd)[1])


# ------------------------------------------------------------------------------------------------ 4. decoupled decay and the average
@pytest.mark.parametrize('decoupled', [False, True])
@pytest.mark.parametrize('n', SIZES)
def test_decoupled_decay_and_ema_over_three_steps(n, decoupled, dev):
    """three consecutive calls on the same device buffers with a new gradient each; after every call p, m, v and ema against the float64
    restatement continued from the DEVICE's state before that call (each step gated on its own)"""
    wd, d, max_norm = 1e-2, 0.9, 0.0
    g, m, v, p0, _ = inputs(n, 1)
    b = Buffers(dev, p0, g, m, v, 0, ema=p0)
    before = b.host()
    for t in (1, 2, 3):
        if t > 1:
            b.g.copy_(torch.from_numpy(np.array(inputs(n, t)[0])))
            before = b.host()
        assert b.call(weight_decay=wd, decoupled=decoupled, ema_decay=d) == FC_OK
        got = b.host()
        assert got['t'] == float(t) and got['stats'].tolist() == [0.0, 1.0, 0.0, 0.0]
        kw = dict(weight_decay=wd, decoupled=decoupled, ema_decay=d)
        state = (before['p'], before['g'], before['m'], before['v'], before['ema'], t - 1, LR)
        want, own = cref.step_ctl(*state, np.float64, **kw), cref.step_ctl(*state, np.float32, **kw)
        assert_within_gate(got, want, own, before['p'], 'decoupled=%d n=%d t=%d' % (decoupled, n, t))
        before = got
    assert not same_bits(got['ema'], got['p']) and not same_bits(got['ema'], p0)


def test_decoupled_decay_differs_from_l2(dev):
    n = 1028
    g, m, v, p0, _ = inputs(n, 1)
    res = []
    for decoupled in (False, True):
        b = Buffers(dev, p0, g, m, v, 0)
        assert b.call(weight_decay=1e-2, decoupled=decoupled) == FC_OK
        res.append(b.host())
    assert not same_bits(res[0]['m'], res[1]['m']) and not same_bits(res[0]['p'], res[1]['p'])
    # decoupled: the moments see the bare gradient (to rounding: the compiler may fuse b1 m + (1-b1) g differently in the two kernels)
    m0 = old_step(dev, p0, g, m, v, 0, n, 0.0)[1]
    assert oref.rel_err(res[1]['m'], m0) < 4e-7                     # (two float32 roundings each, terms of one sign: 2 ulps apart at most)
    assert not np.allclose(res[0]['m'], m0, rtol=1e-3, atol=0)      # L2: the moments see wd p as well


# ------------------------------------------------------------------------------------------------ 5. the skip
@pytest.mark.parametrize('value', [np.nan, np.inf])
@pytest.mark.parametrize('n', SIZES)
def test_nonfinite_gradient_skips_the_step(n, value, dev):
    """one NaN, then one +inf (a value in a buffer) at element 0, at element n-1 and inside the last workgroup's range of the sum of
    squares"""
    t0, d, wd = 7, 0.9, 1e-2
    g, m, v, p0, _ = inputs(n, 1)
    last = (parts_of(n) - 1) * CHUNK
    fresh = Buffers(dev, p0, g, m, v, t0, ema=p0)                  # the finite step from the same state, once
    assert fresh.call(weight_decay=wd, max_norm=1.0, skip_nonfinite=True, ema_decay=d) == FC_OK
    ref = fresh.host()
    for pos in (0, n - 1, last + (n - last) // 2):
        bad = np.array(g)
        bad[pos] = value
        b = Buffers(dev, p0, bad, m, v, t0, ema=p0, n_skipped=5.0)
        assert b.call(weight_decay=wd, max_norm=1.0, skip_nonfinite=True, ema_decay=d) == FC_OK
        got = b.host()
        assert got['t'] == float(t0) and all(same_bits(got[k], a) for k, a in (('p', p0), ('m', m), ('v', v), ('ema', p0))), pos
        assert got['stats'][2:].tolist() == [1.0, 6.0] and not np.isfinite(got['stats'][0]), pos
        # the following finite step is step t0 + 1: the bits of a call that never saw the bad gradient
        b.g.copy_(torch.from_numpy(np.array(g)))
        assert b.call(weight_decay=wd, max_norm=1.0, skip_nonfinite=True, ema_decay=d) == FC_OK
        nxt = b.host()
        assert nxt['t'] == ref['t'] == float(t0 + 1) and nxt['stats'][2:].tolist() == [0.0, 6.0]
        assert all(same_bits(nxt[k], ref[k]) for k in ('p', 'm', 'v', 'ema')) and not same_bits(nxt['p'], p0)
        # without the control the same gradient goes through and spreads
        b = Buffers(dev, p0, bad, m, v, t0, ema=p0, n_skipped=5.0)
        assert b.call(weight_decay=wd, ema_decay=d) == FC_OK
        got = b.host()
        assert got['t'] == float(t0 + 1) and got['stats'][2:].tolist() == [0.0, 5.0]
        assert not np.isfinite(got['p'][pos]) and not np.isfinite(got['m'][pos]) and not np.isfinite(got['ema'][pos]), pos


# ------------------------------------------------------------------------------------------------ 6. squares beyond float32
@pytest.mark.parametrize('n', (4, 1028, N_PAST_TWO, N_MANY))
def test_norm_does_not_overflow(n, dev):
    """every entry 3e38: the float32 squares would be inf, the double ones are not.  The step is taken, the coefficient is finite and
    positive, the parameters stay finite.  (float32(norm) itself is inf here: 3e38 sqrt(n) is beyond float32.  That is reported in
    stats[0] and is not a skip.)  max_norm = 1e6 keeps the coefficient a normal float32 number at every size."""
    _, _, _, p0, _ = inputs(n, 1)
    g = np.full(n, 3e38, np.float32)
    zero = np.zeros(n, np.float32)
    max_norm = 1e6
    b = Buffers(dev, p0, g, zero, zero, 0)
    assert b.call(max_norm=max_norm, skip_nonfinite=True) == FC_OK
    got = b.host()
    coef = got['stats'][1]
    assert got['t'] == 1.0 and got['stats'][2:].tolist() == [0.0, 0.0] and got['stats'][0] == np.inf
    assert np.isfinite(coef) and coef > 0 and cref.ulps(coef, cref.clip_coef(cref.grad_norm(g), max_norm)) <= 1
    assert np.isfinite(got['p']).all() and np.isfinite(got['m']).all() and np.isfinite(got['v']).all()
    kw = dict(max_norm=max_norm, skip_nonfinite=True, coef=coef)
    want, own = (cref.step_ctl(p0, g, zero, zero, None, 0, LR, f, **kw) for f in (np.float64, np.float32))
    assert_within_gate(got, want, own, p0, 'overflow n=%d' % n)


# ------------------------------------------------------------------------------------------------ 7. through the module, eager
@functools.lru_cache(maxsize=None)
def small_mesh(dev):
    """the synthetic sphere of the optimizer's parity test with its stencils and one input, built once: FCPrecomp's area sums are float
    atomics, so two builds may differ in the last bits"""
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.transforms import FCPrecomp
    N, k, C, B, R = 200, 12, 8, 2, 6
    data = sphere_support(N, k).to(dev)
    edges, sten, _, _ = FCPrecomp(B, R, data.epsilon)(data)
    g = torch.Generator().manual_seed(5)
    x = torch.complex(torch.randn(N, C, generator=g), torch.randn(N, C, generator=g)).to(dev)
    return x, edges, sten, C, B, R


def small_net(dev, seed=5):
    """FieldConv(8, 8, band_limit=2, n_rings=6) + TangentNonLin on small_mesh; every call gives the same initial parameters"""
    from fieldconv_amd.nn import FieldConv, TangentNonLin
    x, edges, sten, C, B, R = small_mesh(dev)
    torch.manual_seed(seed)
    net = torch.nn.ModuleDict(dict(conv=FieldConv(C, C, band_limit=B, n_rings=R), nl=TangentNonLin(C))).to(dev)

    def loss_of(net):
        return net['nl'](net['conv'](x, edges, sten)).abs().square().mean()
    return net, loss_of


def flat_of(opt, buf):
    """the entries of a flat buffer that belong to parameters (padding left out), on the host"""
    return np.concatenate([H(buf[o:o + n]) for o, n in zip(opt._offsets, opt._sizes)])


def test_module_eager_with_scheduler_ema_and_checkpoint(dev):
    import copy
    from fieldconv_amd.optim import FusedAdam
    net, loss_of = small_net(dev)
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, decoupled_weight_decay=True, ema_decay=0.9)
    # a first pass measures the gradient norms, so that max_grad_norm sits among them (clipping on in some steps)
    probe_net = copy.deepcopy(net)
    probe = FusedAdam(probe_net.parameters(), skip_nonfinite=True, **kw)
    probe.zero_grad()
    loss_of(probe_net).backward()
    probe.step()
    max_norm = float(np.float32(0.7 * float(probe.grad_norm())))
    opt = FusedAdam(net.parameters(), max_grad_norm=max_norm, **kw)
    assert opt.lr.shape == (1,) and opt.stats.shape == (4,) and opt.lr.is_cuda
    assert [e.shape for e in opt.ema_parameters()] == [p.shape for p in net.parameters()]
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=1, gamma=0.5)
    live = lambda: (flat_of(opt, opt._flat), flat_of(opt, opt._m), flat_of(opt, opt._v), flat_of(opt, opt._ema))     # noqa: E731
    clipped, checkpoint, recorded = 0, None, {}
    for t in range(1, 7):
        lr = opt.param_groups[0]['lr']
        assert lr == pytest.approx(3e-3 * 0.5 ** (t - 1))
        p_b, m_b, v_b, e_b = live()
        opt.zero_grad()
        loss_of(net).backward()
        opt.step()
        sched.step()
        assert float(opt.lr) == float(np.float32(lr))                      # the scheduler's rate reached the device
        g_now = flat_of(opt, opt._grad)
        recorded[t] = H(opt._grad).copy()
        stats = H(opt.stats)
        assert cref.ulps(stats[0], cref.grad_norm(g_now)) <= 1 and cref.ulps(stats[1], cref.clip_coef(cref.grad_norm(g_now), max_norm)) <= 1
        clipped += bool(stats[1] < 1)
        ctl = dict(weight_decay=1e-2, decoupled=True, max_norm=max_norm, ema_decay=0.9, coef=stats[1])
        want, own = (cref.step_ctl(p_b, g_now, m_b, v_b, e_b, t - 1, lr, f, **ctl) for f in (np.float64, np.float32))
        got = dict(zip(('p', 'm', 'v', 'ema'), live()))
        assert float(opt._step) == t
        assert_within_gate(got, want, own, p_b, 'module step %d lr %.3g coef %.4f' % (t, lr, stats[1]))
        if t == 3:
            checkpoint = (copy.deepcopy(opt.state_dict()), copy.deepcopy(net.state_dict()), copy.deepcopy(sched.state_dict()))
    assert clipped >= 1 and float(opt.skipped()[1]) == 0
    # swap_ema: the averaged weights inside, the live bits back afterwards
    p_live, e_live = flat_of(opt, opt._flat), flat_of(opt, opt._ema)
    with opt.swap_ema():
        inside = np.concatenate([H(p.data).reshape(-1) for p in net.parameters()])
        assert same_bits(inside, e_live) and not same_bits(inside, p_live)
    assert same_bits(flat_of(opt, opt._flat), p_live) and same_bits(flat_of(opt, opt._ema), e_live)
    # state_dict round trip: a fresh optimizer resumes after step 3 and arrives at the same bits
    sd, weights, sched_sd = checkpoint
    assert set(sd['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq', 'ema'} and sd['param_groups'][0]['n_skipped'] == 0
    net2, _ = small_net(dev)
    net2.load_state_dict(weights)
    opt2 = FusedAdam(net2.parameters(), max_grad_norm=max_norm, **dict(kw, lr=1.0))
    opt2.load_state_dict(sd)
    assert float(opt2.lr) == float(np.float32(sd['param_groups'][0]['lr'])) and float(opt2._step) == 3
    sched2 = torch.optim.lr_scheduler.StepLR(opt2, step_size=1, gamma=0.5)
    sched2.load_state_dict(sched_sd)
    # (fed the gradients the uninterrupted run recorded: the round trip of the optimizer's state is what is claimed, whatever the order of
    # the convolution's gradient sums in a second run)
    for t in range(4, 7):
        opt2._grad.copy_(torch.from_numpy(recorded[t]))
        opt2.step()
        sched2.step()
    for a, b in ((opt._flat, opt2._flat), (opt._m, opt2._m), (opt._v, opt2._v), (opt._ema, opt2._ema), (opt.lr, opt2.lr)):
        assert same_bits(H(a), H(b))
    # a checkpoint without the average (plain Adam's layout): the average restarts from the parameters
    for st in sd['state'].values():
        del st['ema']
    opt2.load_state_dict(sd)
    assert same_bits(H(opt2._ema), H(opt2._flat))


# ------------------------------------------------------------------------------------------------ 8. under a captured step
def test_captured_step_follows_set_lr(dev):
    """forward + loss + backward() + opt.step() as one StepGraph (a linear graph); the rate changes between replays through set_lr.
    Compared against the eager run of the same sequence from the same start.  The parameters agree bit for bit when the convolution's
    gradients do; they are compared first, and should its unordered sums ever differ between the two runs, the optimizers are compared
    alone on the gradients the graph run recorded -- which is the claim this test is about."""
    import copy
    from fieldconv_amd.optim import FusedAdam
    from fieldconv_amd.utils import StepGraph
    net_g, loss_g = small_net(dev)
    net_e, loss_e = small_net(dev)
    net_e.load_state_dict(copy.deepcopy(net_g.state_dict()))
    # (max_grad_norm far below any gradient norm of this loss: every step is clipped; Adam's update hardly depends on the scale)
    kw = dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, device_lr=True, max_grad_norm=1e-3, skip_nonfinite=True)
    opt_g, opt_e = FusedAdam(net_g.parameters(), **kw), FusedAdam(net_e.parameters(), **kw)

    def train_step(net, loss_of, opt):
        opt.zero_grad()
        loss = loss_of(net)
        loss.backward()
        opt.step()
        return loss.detach()
    warmup = 2
    graphed = StepGraph(lambda: train_step(net_g, loss_g, opt_g), warmup=warmup)        # the warm-up steps are taken, the capture only records
    for _ in range(warmup):
        train_step(net_e, loss_e, opt_e)
    assert float(opt_g._step) == float(opt_e._step) == warmup
    start = [H(b).copy() for b in (opt_g._flat, opt_g._m, opt_g._v, opt_g._step)]
    rates =(3e-3, 1e-3, 0.0, 2e-2)                     # three rates other than the captured one, one of them zero
    grads_equal = True
    recorded = []
    for lr in rates:
        before = H(opt_g._flat)
        opt_g.set_lr(lr)
        graphed.replay()
        opt_e.set_lr(lr)
        train_step(net_e, loss_e, opt_e)
        torch.cuda.synchronize()
        assert float(opt_g.lr) == float(np.float32(lr))
        recorded.append(H(opt_g._grad))
        grads_equal = grads_equal and same_bits(recorded[-1], H(opt_e._grad))
        if lr == 0.0:
            assert same_bits(H(opt_g._flat), before)                          # lr = 0, no weight decay: the delta is exactly zero
        else:
            assert not same_bits(H(opt_g._flat), before)
    assert float(opt_g._step) == float(opt_e._step) == warmup + len(rates)
    print('\ncaptured step: gradient norm %.4g, coefficient %.4g' % (float(opt_g.grad_norm()), float(opt_g.stats[1])))
    assert float(opt_g.skipped()[1]) == 0 and float(opt_g.stats[1]) < 1       # clipping was at work
    if grads_equal:
        for a, b in ((opt_g._flat, opt_e._flat), (opt_g._m, opt_e._m), (opt_g._v, opt_e._v), (opt_g.stats, opt_e.stats)):
            assert same_bits(H(a), H(b))
    else:
        print('\nthe convolution gradients of the replayed and the eager run differ: comparing the optimizers alone')
    # the optimizer alone: an eager optimizer that starts from the state after the warm-up and is fed the gradients the replays
    # recorded arrives at the replays' bits
    opt_r = FusedAdam([torch.nn.Parameter(torch.zeros_like(p)) for p in net_g.parameters()], **kw)
    for buf, state in zip((opt_r._flat, opt_r._m, opt_r._v, opt_r._step), start):
        buf.copy_(torch.from_numpy(state))
    for lr, grad in zip(rates, recorded):
        opt_r.set_lr(lr)
        opt_r._grad.copy_(torch.from_numpy(grad))
        opt_r.step()                                                          # (.grad are the views of _grad: nothing to pack)
    for a, b in ((opt_g._flat, opt_r._flat), (opt_g._m, opt_r._m), (opt_g._v, opt_r._v), (opt_g.stats, opt_r.stats), (opt_g._step, opt_r._step)):
        assert same_bits(H(a), H(b))


def test_step_does_not_write_the_rate_while_capturing(dev):
    """a param_groups lr that moved before the capture is NOT pushed by the captured step (a captured fill would reset the rate on every
    replay); eager, it is; swap_ema refuses inside a capture"""
    from fieldconv_amd.optim import FusedAdam
    p = torch.nn.Parameter(torch.ones(8, device=dev))
    opt = FusedAdam([p], lr=0.5, device_lr=True, ema_decay=0.5)
    p.grad.fill_(1.0)
    opt.step()                                       # eager first (the capture then only records): p = 1 - 0.5
    opt.param_groups[0]['lr'] = 0.25
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        opt.step()
        with pytest.raises(RuntimeError, match='captur'):
            with opt.swap_ema():
                pass
    assert float(opt.lr) == 0.5
    opt.set_lr(0.125)
    graph.replay()
    torch.cuda.synchronize()
    assert float(opt.lr) == 0.125 and float(opt._step) == 2
    assert np.allclose(H(p.data), 0.5 - 0.125, rtol=1e-5)                    # a constant gradient: every Adam step moves by its lr
    opt.param_groups[0]['lr'] = 0.25
    opt.step()                                                               # eager: pushed
    assert float(opt.lr) == 0.25
    opt.set_lr(torch.full((1,), 0.0625, device=dev))                         # a device tensor is copied
    opt.step()
    assert float(opt.lr) == 0.0625


# ------------------------------------------------------------------------------------------------ 9. the defaults
def test_defaults_are_the_old_path(dev):
    from fieldconv_amd.optim import FusedAdam
    n, t = 1028, 1
    g, _, _, p0, _ = inputs(n, t)
    h = oref.HYPER
    for wd in (0.0, 1e-2):
        p = torch.nn.Parameter(torch.from_numpy(np.array(p0)).to(dev))
        opt = FusedAdam([p], h['lr'], (h['beta1'], h['beta2']), h['eps'], wd)
        assert opt.lr is None and opt.stats is None and opt._ema is None and opt._swap is None and opt._ws is None and not opt._ctl
        zero = np.zeros(n, np.float32)
        pp, mm, vv = np.array(p0), zero, zero
        for k in (1, 2, 3):
            p.grad.copy_(torch.from_numpy(np.array(g) * k))
            opt.step()
            pp, mm, vv, counter = old_step(dev, pp, np.array(g) * k, mm, vv, k - 1, n, wd)
            assert same_bits(H(opt._flat), pp) and same_bits(H(opt._m), mm) and same_bits(H(opt._v), vv) and float(opt._step) == counter
        assert 'n_skipped' not in opt.state_dict()['param_groups'][0] and set(opt.state_dict()['state'][0]) == {'step', 'exp_avg', 'exp_avg_sq'}
        with pytest.raises(RuntimeError):
            opt.set_lr(1e-3)
        # the same through the new entry, for the same rate: the controls' neutral setting costs no bits
        q = torch.nn.Parameter(torch.from_numpy(np.array(p0)).to(dev))
        opt_c = FusedAdam([q], h['lr'], (h['beta1'], h['beta2']), h['eps'], wd, device_lr=True)
        for k in (1, 2, 3):
            q.grad.copy_(torch.from_numpy(np.array(g) * k))
            opt_c.step()
        assert same_bits(H(opt_c._flat), H(opt._flat)) and same_bits(H(opt_c._m), H(opt._m))
