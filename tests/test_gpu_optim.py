"""fc_adam_step (csrc/fc_optim.hip) on its own, element by element against the float64 numpy restatement of its formula
(tests/_optim_ref.py, pinned to torch.optim.Adam by tests/test_optim_host.py).

The end-to-end test (test_gpu_parity.py::test_fused_adam_matches_torch_adam) gates the PARAMETERS after six small steps, so an update
wrong by 0.1 % passes it.  Here the kernel is called directly on flat buffers: with p = 0 and no weight decay the result is minus the
update, whose relative error is measured element by element, as are m and v; gradients span 2^-30 .. 2^20 so that sqrt(v) sits on
both sides of eps.  Gate: 4 x the float32 restatement's own error, floor 1e-6."""
import numpy as np
import pytest
import torch

import _optim_ref as oref

pytestmark = pytest.mark.gpu
FC_OK, FC_ERR_BAD_ARGUMENT = 0, -1


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def native_step(dev, p, g, m, v, step_before, n, weight_decay):
    """fc_adam_step on copies of the buffers, the device counter preset to step_before -> (status, p, m, v, counter)"""
    from fieldconv_amd import _lib
    from fieldconv_amd._launch import _p, stream
    t = [torch.from_numpy(np.array(a, np.float32)).to(dev) for a in (p, g, m, v)]
    step = torch.full((1,), float(step_before), dtype=torch.float32, device=dev)
    h = oref.HYPER
    status = _lib.load().fc_adam_step(_p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), _p(step), n, h['lr'], h['beta1'], h['beta2'], h['eps'],
                                      weight_decay, stream())
    torch.cuda.synchronize()
    return status, H(t[0]), H(t[2]), H(t[3]), float(step.item())


@pytest.mark.parametrize('t', oref.STEPS)
@pytest.mark.parametrize('n', oref.SIZES)
def test_adam_step_elementwise(n, t, dev):
    g, m, v, p0, dead = oref.inputs(n, t)
    zero = np.zeros(n, np.float32)
    # -- p = 0, no weight decay: the result is minus the update
    status, p1, m1, v1, counter = native_step(dev, zero, g, m, v, t - 1, n, 0.0)
    assert status == FC_OK and counter == float(t)
    want, own = oref.adam_step(zero, g, m, v, t, 0.0), oref.adam_step(zero, g, m, v, t, 0.0, np.float32)
    line = []
    for label, got, w, o in zip(('update', 'm', 'v'), (p1, m1, v1), want, own):
        err, own_err = oref.rel_err(got, w), oref.rel_err(o, w)
        line.append('%s %.2e (own %.2e, gate %.2e)' % (label, err, own_err, oref.gate_of(own_err)))
        assert err <= oref.gate_of(own_err), (label, line)
    # g = m = v = 0 and no weight decay: nothing moves, bit for bit
    assert dead.any()
    for got, before in ((p1, zero), (m1, m), (v1, v)):
        assert np.array_equal(bits(got)[dead], bits(before)[dead])
    # -- random p, weight decay 1e-2: p against max(|update|, ulp(p))
    wd = 1e-2
    status, p2, m2, v2, counter = native_step(dev, p0, g, m, v, t - 1, n, wd)
    assert status == FC_OK and counter == float(t)
    want, own = oref.adam_step(p0, g, m, v, t, wd), oref.adam_step(p0, g, m, v, t, wd, np.float32)
    floor = np.maximum(np.abs(want[0] - p0.astype(np.float64)), np.spacing(np.abs(p0)).astype(np.float64))
    for label, got, w, o, fl in zip(('p', 'm', 'v'), (p2, m2, v2), want, own, (floor, None, None)):
        if fl is None:
            err, own_err = oref.rel_err(got, w), oref.rel_err(o, w)
        else:
            err, own_err = float((np.abs(got - w) / fl).max()), float((np.abs(o - w) / fl).max())
        line.append('wd %s %.2e (own %.2e, gate %.2e)' % (label, err, own_err, oref.gate_of(own_err)))
        assert err <= oref.gate_of(own_err), (label, line)
    print('\nfc_adam_step n=%d t=%d: %s' % (n, t, '  '.join(line)))


@pytest.mark.parametrize('t', oref.STEPS)
def test_adam_step_opposite_signs(t, dev):
    """m and g with signs of their own, as in training: b1 m + (1-b1) g cancels in places.  m against max(|m|, one ulp of its larger
    term), the update against the same floor carried through the division (update times floor / |m|), v relatively."""
    n = 1028
    g, m, v, _, dead = oref.inputs(n, t, free_signs=True)
    zero = np.zeros(n, np.float32)
    status, p1, m1, v1, counter = native_step(dev, zero, g, m, v, t - 1, n, 0.0)
    assert status == FC_OK and counter == float(t)
    want, own = oref.adam_step(zero, g, m, v, t, 0.0), oref.adam_step(zero, g, m, v, t, 0.0, np.float32)
    fm = oref.term_floor(g, m)
    live = want[1] != 0
    fu = np.where(live, np.abs(want[0]) * fm / np.where(live, np.abs(want[1]), 1.0), 0.0)
    line = []
    for label, got, w, o, fl in zip(('update', 'm', 'v'), (p1, m1, v1), want, own, (fu, fm, None)):
        err, own_err = oref.rel_err(got, w, fl), oref.rel_err(o, w, fl)
        line.append('%s %.2e (own %.2e, gate %.2e)' % (label, err, own_err, oref.gate_of(own_err)))
        assert err <= oref.gate_of(own_err), (label, line)
    for got, before in ((p1, zero), (m1, m), (v1, v)):
        assert np.array_equal(bits(got)[dead], bits(before)[dead])
    print('\nfc_adam_step, signs of their own, n=%d t=%d: %s' % (n, t, '  '.join(line)))


def test_adam_step_refuses_and_skips(dev):
    g, m, v, p0, _ = oref.inputs(8, 1)
    # n = 0: nothing to do, the counter stays
    status, p1, m1, v1, counter = native_step(dev, p0, g, m, v, 5, 0, 1e-2)
    assert status == FC_OK and counter == 5.0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in ((p1, p0), (m1, m), (v1, v)))
    # n = 6: not a whole number of float4 -- refused, nothing written
    status, p1, m1, v1, counter = native_step(dev, p0, g, m, v, 5, 6, 1e-2)
    assert status == FC_ERR_BAD_ARGUMENT and counter == 5.0
    assert all(np.array_equal(bits(a), bits(b)) for a, b in ((p1, p0), (m1, m), (v1, v)))


def test_fused_adam_padding_stays_zero(dev):
    """Parameters of 5, 3 and 1 elements start on 16-byte boundaries: the padding entries of the flat buffers take part in every step
    (one elementwise kernel) and must stay exactly zero, weight decay included; each p.data stays a view of the flat buffer."""
    from fieldconv_amd.optim import FusedAdam
    g = torch.Generator().manual_seed(7)
    ps = [torch.nn.Parameter(torch.randn(k, generator=g).to(dev)) for k in (5, 3, 1)]
    opt = FusedAdam(ps, lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2)
    assert opt._offsets == [0, 8, 12] and opt._n == 16
    pad = torch.ones(16, dtype=torch.bool)
    for o, k in zip(opt._offsets, (5, 3, 1)):
        pad[o:o + k] = False
    before = [p.detach().clone() for p in ps]
    for _ in range(3):
        opt.zero_grad()
        sum((p * p).sum() for p in ps).backward()
        opt.step()
    torch.cuda.synchronize()
    for buf in (opt._flat, opt._m, opt._v, opt._grad):
        assert np.array_equal(bits(H(buf))[pad.numpy()], np.zeros(int(pad.sum()), np.int32))
    lo, hi = opt._flat.data_ptr(), opt._flat.data_ptr() + 4 * opt._n
    for p, o, b in zip(ps, opt._offsets, before):
        assert p.data.data_ptr() == lo + 4 * o and lo <= p.data.data_ptr() < hi
        assert torch.equal(p.data, opt._flat[o:o + p.numel()]) and not torch.equal(p.data, b)
    assert float(opt._step.item()) == 3.0
