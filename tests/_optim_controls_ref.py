"""numpy restatement of fc_adam_step_ctl's decisions and update (include/fieldconv_hip.h, steps b. and c.) on top of
_optim_ref.adam_step:

    S = sum of g^2;  norm = sqrt(S);  skip = skip_nonfinite and S not finite
    coef = float32(min(1, max_norm / (norm + 1e-6)))  (in double, rounded once; 1 without clipping)
    unless skip:  t += 1;  g = coef g;  decoupled: p = p (1 - lr wd), g' = g;  else: g' = g + wd p;  Adam's m, v, p;
                  ema = d ema + (1 - d) p

S is math.fsum of the squares, each exact in double: the correctly rounded sum.  In float64 the update is the reference; in float32, in
the kernel's order of operations, it is the restatement whose own error, times 4, is the gate (_optim_ref.gate_of).  lr, the
hyper-parameters and coef are float32 values on both sides: the kernel reads floats."""
import math

import numpy as np

import _optim_ref as oref


def grad_norm(g):
    """sqrt of the correctly rounded sum of squares, a Python float (double); non-finite entries give inf or nan as the device does"""
    sq = np.asarray(g).astype(np.float64) ** 2                      # a float32 squared in double: exact
    return math.sqrt(math.fsum(sq.tolist())) if np.isfinite(sq).all() else float(np.sqrt(sq.sum()))


def clip_coef(norm_d, max_norm, rounded=True):
    """torch's clip_grad_norm_ coefficient in double, rounded to float32 once (rounded=False: left in double, torch's own value on
    float64 tensors); None or <= 0: no clipping"""
    if max_norm is None or not max_norm > 0:
        return np.float32(1)
    c = float(np.float32(max_norm)) / (norm_d + 1e-6)
    c = c if not c > 1.0 else 1.0                                   # (a NaN stays a NaN, as in torch's clamp)
    return np.float32(c) if rounded else c


def ulps(a, b):
    """distance of two finite float32 values of one sign in units in the last place"""
    a, b = np.float32(a), np.float32(b)
    assert np.isfinite(a) and np.isfinite(b) and (a >= 0) == (b >= 0)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def step_ctl(p, g, m, v, ema, t_before, lr, dtype=np.float64, weight_decay=0.0, decoupled=False, max_norm=None, skip_nonfinite=False,
             ema_decay=None, coef=None):
    """-> dict(p, m, v, ema, t, norm, coef, skipped) after one call that found the counter at t_before.  coef: the coefficient to use,
    as it is, instead of the one computed here (the device's own, when the two may differ in the last place; torch's unrounded one)."""
    f = dtype
    want_norm = skip_nonfinite or (max_norm is not None and max_norm > 0)
    norm_d = grad_norm(g) if want_norm else 0.0
    skipped = bool(skip_nonfinite and not math.isfinite(norm_d))
    coef = clip_coef(norm_d, max_norm) if coef is None else coef
    out = dict(norm=norm_d, coef=coef, skipped=skipped, t=t_before + (0 if skipped else 1))
    p, g, m, v = (np.asarray(a).astype(f) for a in (p, g, m, v))
    ema = None if ema is None else np.asarray(ema).astype(f)
    if skipped:
        out.update(p=p, m=m, v=v, ema=ema)
        return out
    with np.errstate(all='ignore'):
        g = f(coef) * g
        lr32, wd32 = f(np.float32(lr)), f(np.float32(weight_decay))
        if decoupled:
            p = p * (f(1) - lr32 * wd32)
        p, m, v = oref.adam_step(p, g, m, v, out['t'], 0.0 if decoupled else weight_decay, f, lr=lr)
        if ema_decay is not None:
            d = f(np.float32(ema_decay))
            ema = d * ema + (f(1) - d) * p
    assert p.dtype == f and (ema is None or ema.dtype == f)
    out.update(p=p, m=m, v=v, ema=ema)
    return out


def p_floor(p_before, p_ref):
    """what the error of a parameter is measured against: the size of its change, at least one ulp of the parameter (test_gpu_optim)"""
    p_before = np.asarray(p_before, np.float32)
    return np.maximum(np.abs(np.asarray(p_ref, np.float64) - p_before.astype(np.float64)), np.spacing(np.abs(p_before)).astype(np.float64))


def floor_err(got, ref, floor):
    return float((np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)) / floor).max())
