"""Pins the numpy restatement of fc_adam_step_ctl (tests/_optim_controls_ref.py) on the CPU: it is torch's clip_grad_norm_ followed by
torch.optim.Adam / AdamW, its moving average is the plain recurrence, and the optimizer refuses bad controls before it touches a
device.  The new entry points exist and the ABI is still 11."""
import math
import os
import re

import numpy as np
import pytest
import torch

import _optim_controls_ref as cref
import _optim_ref as oref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {'fc_adam_ctl_workspace_bytes', 'fc_adam_step_ctl'}


def test_entry_points_are_declared_bound_and_exported():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES) and 'fc_adam_step' in declared and 'fc_optim.hip' in build.SOURCES
    assert [len(_lib.SIGNATURES[n][1]) for n in sorted(SYMBOLS)] == [1, 13]
    assert len(_lib.SIGNATURES['fc_adam_step'][1]) == 12              # the old entry keeps its signature
    assert [n for n, _ in _lib.FcAdamCtl._fields_] == ['beta1', 'beta2', 'eps', 'weight_decay', 'decoupled', 'max_norm', 'skip_nonfinite',
                                                       'ema_decay']
    lib = _lib.load(build.build_native())
    assert all(hasattr(lib, n) for n in SYMBOLS) and lib.fc_abi_version() == 11
    # the workspace: 256 bytes for the gate, one double per 4096 floats rounded up to 256 bytes (the header's statement)
    for n, parts in ((4, 1), (4096, 1), (4100, 2), (2 * 4096 + 4, 3), (257 * 4096 + 4, 258)):
        assert lib.fc_adam_ctl_workspace_bytes(n) == 256 + (8 * parts + 255) // 256 * 256


def test_argument_checks_need_no_device():
    """null pointers, n not a multiple of 4, a missing or short workspace and an average without a buffer are refused before anything
    is launched; n == 0 is fine"""
    import ctypes
    from fieldconv_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_float * 64)()
    a = ctypes.cast(buf, ctypes.c_void_p)
    ws = ctypes.cast((ctypes.c_char * 1024)(), ctypes.c_void_p)
    ctl = _lib.FcAdamCtl(0.9, 0.999, 1e-8, 0.0, 0, 1.0, 1, -1.0)
    ok = [a, a, a, a, None, a, a, a, ws, 1024, 8, ctl, None]
    BAD, WORKSPACE = -1, -4
    for hole in (0, 1, 2, 3, 5, 6, 7, 11):
        args = list(ok)
        args[hole] = None
        assert lib.fc_adam_step_ctl(*args) == BAD, hole
    assert lib.fc_adam_step_ctl(*(ok[:10] + [6] + ok[11:])) == BAD                          # n & 3
    assert lib.fc_adam_step_ctl(*(ok[:8] + [None] + ok[9:])) == WORKSPACE
    assert lib.fc_adam_step_ctl(*(ok[:9] + [lib.fc_adam_ctl_workspace_bytes(8) - 1] + ok[10:])) == WORKSPACE
    with_ema = _lib.FcAdamCtl(0.9, 0.999, 1e-8, 0.0, 0, 1.0, 1, 0.5)
    assert lib.fc_adam_step_ctl(*(ok[:11] + [with_ema, None])) == BAD                       # ema_decay >= 0 and no ema buffer
    assert lib.fc_adam_step_ctl(*(ok[:4] + [a] + ok[5:11] + [_lib.FcAdamCtl(0.9, 0.999, 1e-8, 0.0, 0, 1.0, 1, 1.0), None])) == BAD
    assert lib.fc_adam_step_ctl(*(ok[:10] + [0] + ok[11:])) == 0                            # n == 0: nothing to do


@pytest.mark.parametrize('decoupled', [False, True])
@pytest.mark.parametrize('weight_decay', [0.0, 1e-2])
def test_restatement_is_torch_clip_then_adam(decoupled, weight_decay):
    """float64 restatement == clip_grad_norm_ + torch.optim.Adam / AdamW on float64 tensors over 5 steps whose gradients grow through
    the clipping threshold (coefficient 1 at first, below 1 later); the coefficient is left in double as torch leaves it"""
    n = 1028
    g0, _, _, p0, _ = oref.inputs(n, 1)
    g0 = np.clip(g0, -4.0, 4.0).astype(np.float32)                   # (moderate sizes: a norm near the threshold)
    h = {k: float(np.float32(x)) for k, x in oref.HYPER.items()}
    wd = float(np.float32(weight_decay))
    max_norm = float(np.float32(2.5)) * cref.grad_norm(g0)
    max_norm = float(np.float32(max_norm))
    p = torch.from_numpy(p0.astype(np.float64)).requires_grad_(True)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=h['lr'], betas=(h['beta1'], h['beta2']), eps=h['eps'], weight_decay=wd)
    pp, mm, vv = p0.astype(np.float64), np.zeros(n), np.zeros(n)
    coefs = []
    for t in range(1, 6):
        g = g0.astype(np.float64) * t
        p.grad = torch.from_numpy(g.copy())
        total = torch.nn.utils.clip_grad_norm_([p], max_norm)
        opt.step()
        norm = math.sqrt(math.fsum((g * g).tolist()))
        assert abs(float(total) - norm) <= 1e-12 * norm
        coef = cref.clip_coef(norm, max_norm, rounded=False)
        coefs.append(coef)
        r = cref.step_ctl(pp, g, mm, vv, None, t - 1, h['lr'], np.float64, weight_decay=wd, decoupled=decoupled, max_norm=max_norm, coef=coef)
        pp, mm, vv = r['p'], r['m'], r['v']
        assert r['t'] == t and not r['skipped']
    assert coefs[0] == 1.0 and coefs[1] == 1.0 and coefs[-1] < 0.6
    assert np.allclose(p.detach().numpy(), pp, rtol=1e-12, atol=1e-15)
    state = opt.state[p]
    assert np.allclose(state['exp_avg'].numpy(), mm, rtol=1e-12, atol=0) and np.allclose(state['exp_avg_sq'].numpy(), vv, rtol=1e-12, atol=0)


def test_rounded_coefficient_is_one_rounding_of_the_double_formula():
    g, _, _, _, _ = oref.inputs(1028, 2)
    norm = cref.grad_norm(g)
    assert norm == math.sqrt(math.fsum((g.astype(np.float64) ** 2).tolist()))
    for factor, clipped in ((0.5, True), (1.0, None), (2.0, False)):          # (1 x: float32(norm) may fall on either side of norm)
        max_norm = np.float32(factor * norm)
        c = cref.clip_coef(norm, max_norm)
        assert c.dtype == np.float32 and c == np.float32(min(1.0, float(max_norm) / (norm + 1e-6))) and c <= 1
        assert clipped is None or (c < 1) == clipped
    assert cref.clip_coef(norm, None) == 1 and cref.clip_coef(norm, 0.0) == 1
    assert math.isnan(cref.clip_coef(float('nan'), 1.0)) and cref.clip_coef(float('inf'), 1.0) == 0
    # non-finite gradients reach the norm
    bad = g.copy()
    bad[7] = np.inf
    assert cref.grad_norm(bad) == math.inf
    bad[9] = np.nan
    assert math.isnan(cref.grad_norm(bad))
    # squares that overflow float32 do not overflow the norm
    assert cref.grad_norm(np.full(1028, 3e38, np.float32)) == pytest.approx(float(np.float32(3e38)) * math.sqrt(1028), rel=1e-14)


def test_ema_recurrence_and_skip():
    n = 64
    g, m, v, p0, _ = oref.inputs(n, 1)
    d = 0.75
    p, mm, vv, ema = p0.astype(np.float64), m.astype(np.float64), v.astype(np.float64), p0.astype(np.float64)
    loop = p0.astype(np.float64)
    for t in range(1, 5):
        r = cref.step_ctl(p, g, mm, vv, ema, t - 1, 3e-3, np.float64, ema_decay=d)
        p, mm, vv, ema = r['p'], r['m'], r['v'], r['ema']
        for i in range(n):                                              # the plain loop
            loop[i] = d * loop[i] + (1 - d) * p[i]
        assert np.array_equal(ema, loop)
    assert not np.array_equal(ema, p)
    # a skipped step: nothing moves, the counter stays; without the control the same gradient goes through
    bad = g.copy()
    bad[3] = np.nan
    r = cref.step_ctl(p, bad, mm, vv, ema, 4, 3e-3, np.float64, ema_decay=d, skip_nonfinite=True)
    assert r['skipped'] and r['t'] == 4 and all(np.array_equal(a, b) for a, b in ((r['p'], p), (r['m'], mm), (r['v'], vv), (r['ema'], ema)))
    r = cref.step_ctl(p, bad, mm, vv, ema, 4, 3e-3, np.float64, ema_decay=d)
    assert not r['skipped'] and r['t'] == 5 and np.isnan(r['p'][3]) and np.isfinite(np.delete(r['p'], 3)).all()
    # the float32 form stays float32 and close
    r32 = cref.step_ctl(p0, g, m, v, p0, 0, 3e-3, np.float32, weight_decay=1e-2, decoupled=True, max_norm=1.0, ema_decay=d)
    r64 = cref.step_ctl(p0, g, m, v, p0, 0, 3e-3, np.float64, weight_decay=1e-2, decoupled=True, max_norm=1.0, ema_decay=d)
    assert all(r32[k].dtype == np.float32 for k in ('p', 'm', 'v', 'ema'))
    assert max(oref.rel_err(r32[k], r64[k]) for k in ('m', 'v', 'ema')) < 1e-5


@pytest.mark.parametrize('kw', [dict(ema_decay=1.0), dict(ema_decay=-0.1), dict(ema_decay=float('nan')), dict(max_grad_norm=0.0),
                                dict(max_grad_norm=-1.0), dict(max_grad_norm=float('nan'))])
def test_constructor_refuses_bad_controls(kw):
    from fieldconv_amd.optim import FusedAdam
    with pytest.raises(ValueError, match=next(iter(kw))):
        FusedAdam([torch.nn.Parameter(torch.zeros(4))], **kw)
