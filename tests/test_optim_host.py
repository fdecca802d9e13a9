"""Pins the numpy restatement of the fused Adam step (tests/_optim_ref.py) on the CPU: it is torch.optim.Adam's arithmetic, and its
float32 form stays close enough to float64 that the gate of tests/test_gpu_optim.py (4 x that error, floor 1e-6) means something."""
import numpy as np
import pytest
import torch

import _optim_ref as oref


@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
def test_restatement_is_torch_adam(weight_decay):
    g, _, _, p0, _ = oref.inputs(1028, 1)
    h = {k: float(np.float32(x)) for k, x in oref.HYPER.items()}
    p = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    opt = torch.optim.Adam([p], lr=h['lr'], betas=(h['beta1'], h['beta2']), eps=h['eps'], weight_decay=float(np.float32(weight_decay)))
    pp, mm, vv = p0.astype(np.float64), np.zeros(g.size), np.zeros(g.size)
    for t in (1, 2, 3):
        p.grad = torch.from_numpy(g.astype(np.float64) * t)
        opt.step()
        pp, mm, vv = oref.adam_step(pp, g.astype(np.float64) * t, mm, vv, t, weight_decay)
    assert np.allclose(p.detach().numpy(), pp, rtol=1e-12, atol=1e-15)
    state = opt.state[p]
    assert np.allclose(state['exp_avg'].numpy(), mm, rtol=1e-12, atol=0) and np.allclose(state['exp_avg_sq'].numpy(), vv, rtol=1e-12, atol=0)


@pytest.mark.parametrize('t', oref.STEPS)
def test_float32_restatement_is_close(t):
    """the update, m and v of the float32 restatement, element by element: the gate cannot become vacuous"""
    for n in oref.SIZES:
        g, m, v, p0, dead = oref.inputs(n, t)
        zero = np.zeros(n, np.float32)
        want, own = oref.adam_step(zero, g, m, v, t, 0.0), oref.adam_step(zero, g, m, v, t, 0.0, np.float32)
        assert all(a.dtype == np.float32 for a in own)
        assert max(oref.rel_err(o, w) for o, w in zip(own, want)) < 1e-4
        assert all(np.all(a[dead] == 0) for a in want)
        # sqrt(v) sits on both sides of eps
        s = np.sqrt(want[2][~dead])
        assert s.min() < 1e-8 < s.max()
