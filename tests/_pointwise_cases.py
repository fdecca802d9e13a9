"""Inputs, references and expected kernel routes for the tests of the pointwise operators -- TangentLin, TangentNonLin (modReLU)
and softAbs (test_pointwise_host.py pins this module on the CPU; test_gpu_pointwise.py runs the kernels on it).

Inputs of a case (N, I, O): complex64 x (N,I) and gy (N,O), float32 Re, Im (O,I) and bias (1,I), from a seeded generator.
  x    N(0,1) entries with max(|re|, |im|) >= 2^-3, about 1 % exact zeros, one all-zero row (zero_row) and up to three planted
       origin-box entries +-2^-44 +- i 2^-45 (planted) in rows pinned to the smallest exponent (special_rows);
  rows x[n] *= 2^a_n, a in A_RANGE, and gy[n] *= 2^d_n, d in D_RANGE: random inside a 16-row block, and every block of two or
       more rows holds both ends of the range.  Powers of two, formed in double: the scaled inputs are exact in fp32, and the
       smallest ordinary entry (2^-3 2^-20 = 2^-23 = 1.19e-7) stays outside the origin box (|re|, |im| < 1e-7);
  bias N(0, 1/4); the first channel's is positive -- a row of x far below every |bias| still has a non-zero modReLU output there
       -- and the second one's negative.

References are complex128, computed from the fp32 inputs with oracle.fieldconv_oracle (softAbs written out here).  The conditions
on the inputs (assert_lin_conditions, assert_nonlin_conditions) are asserted, never relaxed: a case that misses one gets another
seed (SEEDS)."""
import collections
import functools
import re

import numpy as np

from _dynamic_range_cases import rowwise_err          # noqa: F401  (the one shared row-wise measure)
from oracle import fieldconv_oracle as orc

BLOCK = 16                      # vertices per block of the TangentLin kernels (csrc/fc_pointwise.hip)
A_RANGE = (-20, 13)             # x rows
D_RANGE = (-10, 10)             # gy rows
GATE_MARGIN = 1e-4              # modReLU: no entry outside the origin box has |r + b| < GATE_MARGIN r
DEFAULT_CUS = 256               # what the library assumes without a device (csrc/fc_kernels.hpp, kDefaultCUs)
PERTURB_EXP = 40
SEEDS = {(4101, 48, 48): 2}     # (N, I, O) -> seed of a case whose default seed 0 misses a condition (here: three entries near the modReLU gate)


# ---------------------------------------------------------------- TangentLin cases and the route each launch must take
LinCase = collections.namedtuple('LinCase', 'N I O offset fwd bwd')


def lin_cases(cus):
    """name -> LinCase for a device with `cus` compute units.  The forward launch is the (N, K = I, M = O) product, the input
    gradient the transposed (N, K = O, M = I) one; fwd / bwd hold the fields of fc_tangent_lin_describe's line that the case is
    there for (parse_route).  offset = 1: x and gy are views one complex element off a 16-byte boundary.  With b = ceil(N / 16)
    blocks: the split staged kernel and the direct kernel walk min(b, 4 cus) blocks at a time, the unsplit staged kernel
    4 min(ceil(b / 4), 4 cus); split needs M > 16 and b <= 8 cus; direct needs M > 16, K % 8 == 0 and aligned operands."""
    staged = lambda split, loads, tiles, **kw: dict(kernel='staged', split=split, loads=loads, tiles=tiles, **kw)
    direct = lambda **kw: dict(kernel='direct', **kw)
    n_split2 = BLOCK * (4 * cus + 3) - 5            # 4 cus + 3 blocks, the last one ragged: second trip of the split kernel
    n_unsplit = BLOCK * 8 * cus + 21                # 8 cus + 2 blocks: too many for the split
    n_unsplit2 = BLOCK * 16 * cus + 7               # 16 cus + 1 blocks: second trip of the unsplit kernel
    n_direct2 = BLOCK * 4 * cus + 9                 # 4 cus + 1 blocks: second trip of the direct kernel
    big = 69632                                     # 2 * 64 * (128 + 8) * 4 bytes of LDS: M in 49..64, K in 57..64
    cases = {
        'split-trip2': LinCase(n_split2, 20, 24, 0, staged(1, 'vector', 2, kchunks=1, trips=2), direct(trips=2)),
        'split-trip2-T': LinCase(n_split2, 24, 20, 0, direct(trips=2), staged(1, 'vector', 2, kchunks=1, trips=2)),
        'unsplit-4tiles': LinCase(n_unsplit, 20, 50, 0, staged(0, 'vector', 4, kchunks=1, trips=1), staged(0, 'vector', 2, kchunks=2, trips=1)),
        'unsplit-4tiles-T': LinCase(n_unsplit, 50, 20, 0, staged(0, 'vector', 2, kchunks=2, trips=1), staged(0, 'vector', 4, kchunks=1, trips=1)),
        'unsplit-2tiles': LinCase(n_unsplit, 20, 17, 0, staged(0, 'vector', 2, kchunks=1), staged(0, 'scalar', 2, kchunks=1)),
        'unsplit-trip2': LinCase(n_unsplit2, 12, 40, 0, staged(0, 'vector', 3, trips=2), staged(0, 'vector', 1, trips=2)),
        'scalar-trip2': LinCase(n_unsplit2, 5, 7, 0, staged(0, 'scalar', 1, trips=2), staged(0, 'scalar', 1, trips=2)),
        'misaligned-trip2': LinCase(n_unsplit2, 16, 16, 1, staged(0, 'scalar', 1, trips=2), staged(0, 'scalar', 1, trips=2)),
        'scalar-chunk2': LinCase(200, 63, 20, 0, staged(1, 'scalar', 2, kchunks=2), staged(1, 'vector', 4, kchunks=1)),
        'scalar-chunk2-T': LinCase(200, 20, 63, 0, staged(1, 'vector', 4, kchunks=1), staged(1, 'scalar', 2, kchunks=2)),
        'scalar-chunk2-odd': LinCase(200, 49, 33, 0, staged(1, 'scalar', 3, kchunks=2), staged(1, 'scalar', 4, kchunks=1)),
        'lds-forward': LinCase(200, 60, 64, 0, staged(1, 'vector', 4, kchunks=2, lds=big), direct()),
        'lds-T': LinCase(200, 64, 60, 0, direct(), staged(1, 'vector', 4, kchunks=2, lds=big)),
        'lds-misaligned': LinCase(200, 64, 64, 1, staged(1, 'scalar', 4, kchunks=2, lds=big), staged(1, 'scalar', 4, kchunks=2, lds=big)),
        'direct-k8': LinCase(100, 8, 17, 0, direct(trips=1), staged(0, 'scalar', 1, kchunks=1)),
        'direct-k64': LinCase(100, 64, 64, 0, direct(), direct()),
        'direct-trip2': LinCase(n_direct2, 8, 64, 0, direct(trips=2), staged(0, 'vector', 1, kchunks=2, trips=1)),
    }
    for n in (1, 15, 16, 17):
        cases['edge-staged-N%d' % n] = LinCase(n, 20, 24, 0, staged(1, 'vector', 2, trips=1), direct(trips=1))
        cases['edge-direct-N%d' % n] = LinCase(n, 48, 48, 0, direct(trips=1), direct(trips=1))
    return cases


LIN_NAMES = tuple(lin_cases(DEFAULT_CUS))
CONTAINMENT_NAMES = ('split-trip2', 'unsplit-4tiles', 'scalar-trip2', 'direct-k64')
GEMM_F64_CASE = (130, 7, 70)            # _TangentLinGemmFn on complex128

NONLIN_SHAPES = [(7, 1), (600, 100), (600, 256), (600, 257), (300, 300), (4101, 48), (5, 130)]         # (N, C), fp32
NONLIN_F64_SHAPES = [(1, 1), (64, 65), (65, 300), (1000, 7)]


def parse_route(line):
    """fc_tangent_lin_describe's line as a dict: kernel 'direct' | 'staged', loads as text, every other field an int."""
    words = line.split()
    out = {'kernel': words[0]}
    for w in words[1:]:
        key, value = w.split('=')
        out[key] = int(value) if re.fullmatch(r'-?\d+', value) else value
    return out


def route_mismatch(found, expected):
    """The fields of `expected` that `found` (parse_route) does not show."""
    return {k: (found.get(k), v) for k, v in expected.items() if found.get(k) != v}


# ---------------------------------------------------------------- the generator
def special_rows(N):
    """Rows that carry the planted origin-box entries, pinned to the smallest exponent: odd rows, so never a block's first row."""
    return np.array(sorted({min(r, N - 1) for r in (1, (N // 2) | 1, (3 * N // 4) | 1)}))


def zero_row(N):
    """The all-zero row of x: an even row, or None where there is no room for one."""
    return min(6, (N - 1) // 2 * 2) if N >= 3 else None


def planted(N, I):
    """[(row, column)] of the planted origin-box entries."""
    if N * I < 4:
        return []
    rows = special_rows(N)
    return sorted({(int(rows[k % rows.size]), c) for k, c in enumerate((0, I // 2, I - 1))})


@functools.lru_cache(maxsize=None)
def exponents(N):
    """(a, d): the exponents of the rows of x and of gy."""
    rng = np.random.default_rng([N, 7])
    a = rng.integers(A_RANGE[0], A_RANGE[1] + 1, N)
    d = rng.integers(D_RANGE[0], D_RANGE[1] + 1, N)
    a[0::BLOCK], d[0::BLOCK] = A_RANGE[1], D_RANGE[1]
    a[1::BLOCK], d[1::BLOCK] = A_RANGE[0], D_RANGE[0]
    a[special_rows(N)] = A_RANGE[0]
    return a, d


@functools.lru_cache(maxsize=None)
def base(N, I, O):
    """Unscaled x0 (N,I), gy0 (N,O) complex64; Re, Im (O,I) and bias (1,I) float32."""
    rng = np.random.default_rng([N, I, O, SEEDS.get((N, I, O), 0)])
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x = cplx(N, I)
    small = np.maximum(np.abs(x.real), np.abs(x.imag)) < 0.125
    x[small] = (np.where(x.real[small] < 0, -0.125, 0.125) + 1j * x.imag[small]).astype(np.complex64)
    x[rng.random((N, I)) < 0.01] = 0
    z = zero_row(N)
    assert z is None or z not in special_rows(N)
    if z is not None:
        x[z] = 0
    for k, (n, c) in enumerate(planted(N, I)):
        x[n, c] = complex((-1) ** k * 2.0 ** -44, (-1) ** c * 2.0 ** -45)
    gy = cplx(N, O)
    Re, Im = rng.standard_normal((O, I)).astype(np.float32), rng.standard_normal((O, I)).astype(np.float32)
    bias = (0.5 * rng.standard_normal((1, I))).astype(np.float32)
    bias[0, 0] = abs(bias[0, 0])
    if I > 1:
        bias[0, 1] = -abs(bias[0, 1])
    return x, gy, Re, Im, bias


@functools.lru_cache(maxsize=None)
def inputs(N, I, O):
    """x, gy (rows scaled), Re, Im, bias -- read-only."""
    x0, gy0, Re, Im, bias = base(N, I, O)
    a, d = exponents(N)
    x = (x0.astype(np.complex128) * np.ldexp(1.0, a)[:, None]).astype(np.complex64)
    gy = (gy0.astype(np.complex128) * np.ldexp(1.0, d)[:, None]).astype(np.complex64)
    out = (x, gy, Re, Im, bias)
    for t in out:
        t.setflags(write=False)
    return out


def origin_box(x):
    return orc.is_origin(x)


# ---------------------------------------------------------------- references (complex128, from the fp32 inputs)
@functools.lru_cache(maxsize=None)
def lin_reference(N, I, O):
    """(y, gx, gRe, gIm) of TangentLin."""
    x, gy, Re, Im, _ = inputs(N, I, O)
    x, gy, Re, Im = x.astype(np.complex128), gy.astype(np.complex128), Re.astype(np.float64), Im.astype(np.float64)
    out = (orc.tangent_lin_forward(x, Re, Im),) + tuple(orc.tangent_lin_backward(x, Re, Im, gy))
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def nonlin_reference(N, C):
    """(y, gx, gbias (1,C)) of TangentNonLin on inputs(N, C, C)."""
    x, gy, _, _, bias = inputs(N, C, C)
    x, gy, bias = x.astype(np.complex128), gy.astype(np.complex128), bias.astype(np.float64)
    gx, gb = orc.tangent_nonlin_backward(x, bias, gy)
    return orc.tangent_nonlin_forward(x, bias), gx, np.asarray(gb)


@functools.lru_cache(maxsize=None)
def soft_abs_reference(N, C):
    """(y, gx) of softAbs on the same x with the cotangent Re gy: |x| and g x / |x| outside the origin box, 0 inside."""
    x, gy = inputs(N, C, C)[:2]
    x, g = x.astype(np.complex128), gy.real.astype(np.float64)
    box = origin_box(x)
    r = np.where(box, 1.0, np.abs(x))
    return np.where(box, 0.0, np.abs(x)), np.where(box, 0.0, g * x / r)


def nonlin_reference_longdouble(N, C):
    """(y, gx, gbias) of TangentNonLin in numpy's longdouble, real and imaginary parts apart, from the complex128 / float64 values
    of inputs(N, C, C): the yardstick of the double-precision kernels."""
    x, gy, _, _, bias = inputs(N, C, C)
    L = np.longdouble
    xr, xi, gr_, gi_ = x.real.astype(L), x.imag.astype(L), gy.real.astype(L), gy.imag.astype(L)
    b = np.broadcast_to(bias.astype(L), xr.shape)
    box = (np.abs(xr) < L(1e-7)) & (np.abs(xi) < L(1e-7))
    r = np.where(box, L(1), np.sqrt(xr * xr + xi * xi))
    ex, ey = xr / r, xi / r
    act = (r + b) > 0
    f = np.where(act, r + b, L(0))
    y = np.where(box, xr, f * ex), np.where(box, xi, f * ey)
    g_rad, g_tan = gr_ * ex + gi_ * ey, gi_ * ex - gr_ * ey
    rad, tan = np.where(act, g_rad, L(0)), f / r * g_tan
    gx = np.where(box, gr_, ex * rad - ey * tan), np.where(box, gi_, ey * rad + ex * tan)
    gb = np.where(box, L(0), rad).sum(axis=0).reshape(1, C)
    return y, gx, gb


# ---------------------------------------------------------------- conditions on the inputs
def assert_box_is_the_planted_set(N, I, O):
    x0 = base(N, I, O)[0]
    x = inputs(N, I, O)[0]
    box = origin_box(x)
    assert box.sum() == (x0 == 0).sum() + len(planted(N, I)), (N, I, O)
    assert all(box[n, c] and x[n, c] != 0 for n, c in planted(N, I))


def assert_rows_nonzero(ref, N, what):
    zero = np.abs(np.asarray(ref).reshape(N, -1)).max(axis=1) == 0
    allowed = np.zeros(N, bool)
    if zero_row(N) is not None:
        allowed[zero_row(N)] = True
    assert not (zero & ~allowed).any(), (what, np.flatnonzero(zero & ~allowed))


def assert_lin_conditions(N, I, O):
    assert_box_is_the_planted_set(N, I, O)
    y, gx, gRe, gIm = lin_reference(N, I, O)
    assert_rows_nonzero(y, N, 'y')
    assert_rows_nonzero(gx, N, 'gx')
    if zero_row(N) is not None:
        assert not y[zero_row(N)].any()


def assert_nonlin_conditions(N, C):
    assert_box_is_the_planted_set(N, C, C)
    x, _, _, _, bias = inputs(N, C, C)
    r = np.abs(x.astype(np.complex128))
    out = ~origin_box(x)
    near = out & (np.abs(r + bias.astype(np.float64)) < GATE_MARGIN * r)
    assert not near.any(), ('modReLU gate decided by rounding', N, C, int(near.sum()))         # zero exclusions
    y, gx, gb = nonlin_reference(N, C)
    assert_rows_nonzero(y, N, 'y')
    assert_rows_nonzero(gx, N, 'gx')
    # softAbs is zero inside the origin box: its zero rows are the rows that lie in the box entirely (the all-zero row; with one
    # channel also the rows of the planted entries), and those must come out as exact zeros
    boxed = origin_box(x).all(axis=1)
    for ref in soft_abs_reference(N, C):
        assert np.array_equal(np.abs(ref).max(axis=1) == 0, boxed)
    assert boxed.sum() == (zero_row(N) is not None) + (len(planted(N, C)) if C == 1 else 0)


# ---------------------------------------------------------------- containment
def perturbed_rows(N):
    """The last row of every sixth 16-row block -- the row behind it starts the next block -- plus row N - 1, which the kernels'
    clamped loads of rows beyond the mesh read."""
    return np.unique(np.concatenate([np.arange(BLOCK - 1, N - 1, 6 * BLOCK), [N - 1]]))
