"""numpy restatement of fc_adam_step (the formula in the header of csrc/fc_optim.hip; torch.optim.Adam's arithmetic: L2 weight decay,
no amsgrad) and the inputs of tests/test_gpu_optim.py.

    g' = g + wd p;  m = b1 m + (1-b1) g';  v = b2 v + (1-b2) g'^2;  p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

In float64 it is the reference; in float32, with the kernel's order of operations, it is the float32 restatement whose own error,
times 4, is the gate.  The hyper-parameters are rounded to float32 first on both sides: the ABI takes floats."""
import numpy as np

HYPER = dict(lr=3e-3, beta1=0.9, beta2=0.999, eps=1e-8)
SIZES = (4, 8, 1020, 1024, 1028)            # either side of one 256-thread workgroup of float4
STEPS = (1, 2, 10, 1000)
E_RANGE = (-30, 20)
FLOOR = 1e-6


def adam_step(p, g, m, v, t, weight_decay, dtype=np.float64, lr=HYPER['lr'], beta1=HYPER['beta1'], beta2=HYPER['beta2'], eps=HYPER['eps']):
    """(p, m, v) after step number t (1-based), every operation in `dtype`"""
    f = dtype
    lr, b1, b2, eps, wd = (f(np.float32(h)) for h in (lr, beta1, beta2, eps, weight_decay))
    p, g, m, v = (np.asarray(a).astype(f) for a in (p, g, m, v))
    one, t = f(1), f(t)
    bc1, bc2_sqrt = one - b1 ** t, np.sqrt(one - b2 ** t)
    gk = g + wd * p
    m = b1 * m + (one - b1) * gk
    v = b2 * v + (one - b2) * gk * gk
    p = p - (lr / bc1) * (m / (np.sqrt(v) / bc2_sqrt + eps))
    assert p.dtype == m.dtype == v.dtype == f
    return p, m, v


def inputs(n, t, free_signs=False):
    """g, m, v (float32): gradients N(0,1) 2^e with e in E_RANGE element by element, moments of the same scale (sqrt(v) ~ 2^e: next to
    eps = 1e-8 at the small end, so the place of eps in the denominator is decided), about 5 % exact zeros in g, and `dead` elements
    with g = m = v = 0.  p0: N(0,1) parameters for the weight-decay run.  m and p0 carry the sign of g (where g is zero: the same
    sign as each other), so that neither g + wd p nor b1 m + (1-b1) g' cancels: a cancelling sum keeps the rounding of its terms,
    which depends on whether the compiler fuses the multiply-adds -- the conditioning of the inputs, not the arithmetic under test.
    free_signs: m and p0 with signs of their own, the usual case in training; b1 m + (1-b1) g then cancels in places, and the errors of
    m and of the update are measured against max(|ref|, the ulp of the larger term) (term_floor)."""
    rng = np.random.default_rng([n, t])
    e = rng.integers(E_RANGE[0], E_RANGE[1] + 1, n)
    e[:2] = E_RANGE
    g = np.ldexp(rng.standard_normal(n), e).astype(np.float32)
    sign = np.where(g < 0, -1.0, 1.0)
    if free_signs:
        sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    m = (sign * np.ldexp(np.abs(rng.standard_normal(n)), e)).astype(np.float32)
    v = np.ldexp(rng.standard_normal(n) ** 2, 2 * e).astype(np.float32)
    p0 = (sign * np.abs(rng.standard_normal(n))).astype(np.float32)
    zero = rng.random(n) < 0.05
    zero[2:4] = True
    g[zero] = 0
    dead = zero & (np.arange(n) % 2 == 1)
    m[dead], v[dead] = 0, 0
    assert (v >= 0).all() and dead.any() and (zero & ~dead).any() and np.isfinite(g).all() and (v[~dead] > 0).all()
    assert free_signs or (np.all(g * m >= 0) and np.all(g * p0 >= 0) and np.all(m * p0 >= 0))
    assert not free_signs or (g * m < 0).mean() > 0.3
    return g, m, v, p0, dead


def term_floor(g, m, beta1=HYPER['beta1']):
    """One float32 ulp of the larger of the two terms of b1 m + (1-b1) g (no weight decay): what rounding leaves in their sum however far
    it cancels"""
    b1 = np.float64(np.float32(beta1))
    big = np.maximum(np.abs(b1 * np.asarray(m, np.float64)), np.abs((1 - b1) * np.asarray(g, np.float64)))
    return np.spacing(big.astype(np.float32)).astype(np.float64)


def rel_err(got, ref, floor=None):
    """max over elements of |got - ref| / max(|ref|, floor); where ref is zero (and there is no floor) got must be zero"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    den = np.abs(ref) if floor is None else np.maximum(np.abs(ref), floor)
    assert np.all(got[den == 0] == 0)
    return float((np.abs(got - ref)[den > 0] / den[den > 0]).max(initial=0.0))


def gate_of(own):
    return max(4 * own, FLOOR)
