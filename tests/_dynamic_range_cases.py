"""Inputs and exact references for the row-by-row dynamic-range tests (test_dynamic_range_host.py pins this generator on the
CPU; the GPU tests of the per-row scaling sites run the kernels on it).

One base problem per shape: FCPrecomp stencils on sphere_support with one vertex without out-edges and one without in-edges,
N(0,1) features with exact zeros, one all-zero feature row, a few origin-box entries, a filter with one all-zero output row and
one all-zero input column.  The base problem is then scaled by POWERS OF TWO only:

    x[j]   *= 2^(a_j + gX)        per vertex, and a global exponent
    gy[n]  *= 2^(d_n + gG)        per vertex, and a global exponent
    W[o,i] *= 2^(b_o + c_i)       per output row and per input column (zonal / spherical rows and columns on the parameter path)

Every scaled input is exact in fp32 (asserted by the host test).  The per-vertex and per-channel exponents (a `layout`) mix
inside the sums, so each (shape, layout) is its own problem; the GLOBAL exponents are pure factors of the answer:

    y ~ 2^gX,   gx ~ 2^gG,   gW ~ 2^(gX + gG)

with one proviso.  The operator is not homogeneous in x: entries inside the origin box (|re|, |im| < 1e-7, an ABSOLUTE bound)
are not rotated and carry no angular gradient term.  So there are two regimes, each with its own reference:

    'rot'  gX >= 0: every entry is outside the box, except exact zeros and the planted origin-box entries -- those sit in rows
           pinned to the smallest exponent and are +-2^-44 / +-2^-45, inside the box for every gX of this regime;
    'lin'  gX tiny: every entry is inside the box.  Evaluated by the oracle on x * 2^-200 (complex128 has the range) and scaled back.

The reference of a (shape, layout, regime, filter kind) is computed ONCE in complex128 with oracle.fieldconv_oracle and cached;
every global-exponent combination rescales it."""
import functools

import numpy as np

from oracle import fieldconv_oracle as orc

TILE = 16                       # vertices per tile of every record-driven kernel (csrc/fc_tile.hpp, kTile)
FLOOR_EXP = -100                # a row whose reference maximum is below 2^-100 is left out of the row-wise measures
MAX_EXCLUDED = 0.02             # ... and at most this share of the rows of any tensor

# N, k, I, O, B, R
SHAPES = {
    'rec400': (400, 12, 48, 40, 2, 6),          # frequency-major forward + data / filter kernel pair, on records
    'split60': (60, 40, 48, 40, 2, 6),          # few tiles, long rows: the edge split (parts > 1)
    'param400': (400, 12, 24, 24, 2, 6),        # parameter path
    'ring4400': (4400, 6, 48, 48, 2, 6),        # ring-major forward (just over one tile per CU) and streaming backward, default layer
    'ring4400pad': (4400, 6, 40, 40, 2, 6),     # K padded
    'ring5000': (5000, 7, 64, 64, 3, 6),
    'stream3100': (3100, 8, 16, 32, 1, 4),      # smallest streaming geometry
    'stream3075': (3075, 16, 64, 64, 3, 6),     # two walks, the k range in halves
}
# further shapes on the same generator, registered by sibling case modules (_wide_runtime_cases.py); kept apart from SHAPES so that
# the tests that sweep SHAPES keep their cases.  EXTRA_MESHES: name -> function(name) returning what mesh() returns, for shapes whose
# stencil is not FCPrecomp's.
EXTRA_SHAPES = {}
EXTRA_MESHES = {}


def dims(name):
    return SHAPES[name] if name in SHAPES else EXTRA_SHAPES[name]


SMALLEST = 'split60'
STREAMING_SHAPES = ('ring4400', 'stream3100', 'stream3075')         # N >= 3072: the streaming backward in the default mode
CONTAINMENT_SHAPES = ('ring4400', 'stream3100', 'split60')          # ring forward + streaming backward, streaming backward, edge split
PARAM_CASES = [('param400', 0), ('param400', 1), ('param400', 2), ('ring4400', 1)]         # (shape, filter type) of the parameter path
PARAM_GLOBALS = ('unit-unit', 'unit-tiny', 'tiny-unit', 'tiny-tiny', 'huge-huge')

A_RANGE = (-20, 13)             # x rows
D_RANGE = (-10, 10)             # gy rows
B_RANGE = (-10, 6)              # filter output rows
C_RANGE = (-8, 8)               # filter input columns
LAYOUTS = ('random', 'tiles')
# containment: the random layout with the rows of perturbed_set() times 2^40 in x, or in gy
PERTURBED_LAYOUTS = {'random+xP': 'random', 'random+gP': 'random'}
PERTURB_EXP = 40

# global exponents (gX, gG).  The smallest row of gW is about 2^(gX + gG + 19), and it must stay above 2^-100; x is inside the origin
# box from 2^-39 down; rows of H are at most 2^(gG + 12.1), and the square of their inverse scale is zero in fp32 once they are below
# 2^-62.  So -85 on gy alone, and -76 beside the tiny x of the tiny/tiny pair, put EVERY row of H below 2^-62
# (test_dynamic_range_host.py asserts it).
X_TINY, X_HUGE = -60, 40
G_TINY, G_HUGE = -85, 30
GLOBALS = {
    'unit-unit': (0, 0), 'unit-tiny': (0, G_TINY), 'unit-huge': (0, G_HUGE),
    'tiny-unit': (X_TINY, 0), 'tiny-tiny': (-42, -76), 'tiny-huge': (X_TINY, G_HUGE),
    'huge-unit': (X_HUGE, 0), 'huge-tiny': (X_HUGE, G_TINY), 'huge-huge': (X_HUGE, G_HUGE),
}


def regime_of(gX):
    return 'lin' if gX < 0 else 'rot'


def rowwise_err(a, ref):
    """max over rows of max|delta_row| / max|ref_row| (rows of zeros in ref must be exactly zero)."""
    a, ref = np.asarray(a), np.asarray(ref)
    a, ref = a.reshape(a.shape[0], -1), ref.reshape(ref.shape[0], -1)
    num = np.abs(a - ref).max(axis=1)
    den = np.abs(ref).max(axis=1)
    assert np.all(num[den == 0] == 0)
    return float((num[den > 0] / den[den > 0]).max(initial=0.0))


def row_max(t):
    t = np.asarray(t)
    return np.abs(t.reshape(t.shape[0], -1)).max(axis=1)


def excluded_rows(ref):
    """Rows left out of a row-wise measure: nonzero in the reference, but below 2^FLOOR_EXP (a zero row stays in: it must come out as zeros)."""
    m = row_max(ref)
    return (m > 0) & (m < 2.0 ** FLOOR_EXP)


def measured_err(got, ref, rows=None):
    """rowwise_err over the rows that count (all but excluded_rows; `rows`: a further boolean selection)."""
    keep = ~excluded_rows(ref)
    if rows is not None:
        keep &= rows
    return rowwise_err(np.asarray(got)[keep], np.asarray(ref)[keep])


@functools.lru_cache(maxsize=None)
def mesh(name):
    """(edges (E,2) int64, sten (E,R,F) complex64) as numpy, built on the CPU; vertex N-2 has no out-edges, vertex 37 no in-edges."""
    from fieldconv_amd.data import sphere_support
    from oracle.torch_composites import FCPrecomp
    if name in EXTRA_MESHES:
        return EXTRA_MESHES[name](name)
    N, k, I, O, B, R = dims(name)
    no_out, no_in = N - 2, 37
    data = sphere_support(N, k=k, seed=N + k, support='p95')
    keep = (data.supp_edges[:, 0] != no_out) & (data.supp_edges[:, 1] != no_in)
    for attr in ('supp_edges', 'logMag', 'logAng', 'xp'):
        setattr(data, attr, getattr(data, attr)[keep].contiguous())
    edges, sten = FCPrecomp(B, R, data.epsilon)(data)[:2]
    edges, sten = edges.numpy(), sten.numpy()
    assert not (edges[:, 0] == no_out).any() and not (edges[:, 1] == no_in).any()
    return edges, sten, no_out, no_in


ZERO_X_ROW, ZERO_W_ROW, ZERO_W_COL = 7, 3, 5


def special_rows(name):
    """Rows that carry the planted origin-box entries (pinned to the smallest a_j): one per quarter of the mesh."""
    N = dims(name)[0]
    return np.array([1, N // 4 + 2, N // 2 + 3, (3 * N) // 4 + 5])


@functools.lru_cache(maxsize=None)
def base(name):
    """x0 (N,I), gy0 (N,O), W0 (O,I,R,F) complex64, and the module parameters of the three filter types (float32)."""
    N, k, I, O, B, R = dims(name)
    F = 2 * B + 1
    rng = np.random.default_rng([N, k, I, O])
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    x = cplx(N, I)
    # no ordinary entry may fall into the origin box at the smallest exponent: max(|re|, |im|) >= 2^-3 (2^-23 = 1.19e-7 > 1e-7)
    small = np.maximum(np.abs(x.real), np.abs(x.imag)) < 0.125
    x[small] = (np.where(x.real[small] < 0, -0.125, 0.125) + 1j * x.imag[small]).astype(np.complex64)
    x[rng.random((N, I)) < 0.01] = 0
    x[ZERO_X_ROW] = 0
    for n, j in enumerate(special_rows(name)):          # +-2^-44 +- i 2^-45: inside the box at every exponent of the 'rot' regime
        for c in (0, I // 2, I - 1):
            x[j, c] = complex((-1) ** n * 2.0 ** -44, (-1) ** c * 2.0 ** -45)
    gy = cplx(N, O)
    W = (cplx(O, I, R, F) / np.sqrt(I * R)).astype(np.complex64)
    W[ZERO_W_ROW] = 0
    W[:, ZERO_W_COL] = 0
    real = lambda *s: (rng.standard_normal(s) / np.sqrt(I * R)).astype(np.float32)
    params = {}
    for ftype in (0, 1, 2):
        z = real(O, I, R) if ftype < 2 else real(O, I, R, 2)
        s = real(O, I, R, B if ftype < 2 else 2 * B, 2)
        p = rng.uniform(-np.pi, np.pi, (O, I, B + 1)).astype(np.float32) if ftype == 1 else np.zeros((O, I, B + 1), np.float32)
        z[ZERO_W_ROW], s[ZERO_W_ROW] = 0, 0
        z[:, ZERO_W_COL], s[:, ZERO_W_COL] = 0, 0
        params[ftype] = (z, s, p)
    return x, gy, W, params


@functools.lru_cache(maxsize=None)
def exponents(name, layout):
    """(a (N,), d (N,), b (O,), c (I,)) integer exponents of one layout."""
    N, k, I, O, B, R = dims(name)
    if layout in PERTURBED_LAYOUTS:
        a, d, b, c = exponents(name, PERTURBED_LAYOUTS[layout])
        a, d = a.copy(), d.copy()
        (a if layout.endswith('xP') else d)[perturbed_set(name)] += PERTURB_EXP
        return a, d, b, c
    rng = np.random.default_rng([N, O, LAYOUTS.index(layout)])
    b = rng.integers(B_RANGE[0], B_RANGE[1] + 1, O)
    c = rng.integers(C_RANGE[0], C_RANGE[1] + 1, I)
    b[:2], c[:2] = B_RANGE, C_RANGE
    tile = np.arange(N) // TILE
    if layout == 'random':
        a = rng.integers(A_RANGE[0], A_RANGE[1] + 1, N)
        d = rng.integers(D_RANGE[0], D_RANGE[1] + 1, N)
        a[::TILE] = A_RANGE[1]                            # every tile spans the whole range, the ragged last one included
        a[N - 1] = A_RANGE[0]
        d[::TILE] = D_RANGE[1]
        d[N - 1] = D_RANGE[0]
    else:
        # whole tiles tiny next to whole tiles huge; d with twice the period, so that all four pairings occur
        a = np.where(tile % 2 == 0, A_RANGE[1], A_RANGE[0])
        d = np.where((tile // 2) % 2 == 0, D_RANGE[1], D_RANGE[0])
    a[special_rows(name)] = A_RANGE[0]
    return a, d, b, c


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e))


def scaled_inputs(name, layout, gX, gG):
    """x, gy, W complex64 of the scaled problem (products formed in double precision: exact, the host test asserts it)."""
    x0, gy0, W0, _ = base(name)
    a, d, b, c = exponents(name, layout)
    x = (x0.astype(np.complex128) * _pow2(a + gX)[:, None]).astype(np.complex64)
    gy = (gy0.astype(np.complex128) * _pow2(d + gG)[:, None]).astype(np.complex64)
    W = (W0.astype(np.complex128) * _pow2(b[:, None] + c[None, :])[:, :, None, None]).astype(np.complex64)
    return x, gy, W


def scaled_params(name, layout, ftype):
    """zonal, spherical, phase float32 with rows o and columns i scaled by 2^(b_o + c_i) (the phases are angles: unscaled)."""
    z, s, p = base(name)[3][ftype]
    _, _, b, c = exponents(name, layout)
    f = _pow2(b[:, None] + c[None, :]).astype(np.float32)
    return z * f.reshape(f.shape + (1,) * (z.ndim - 2)), s * f.reshape(f.shape + (1,) * (s.ndim - 2)), p


def filter_of(name, layout, wkind):
    """The complex128 effective filter of the scaled problem: wkind 'explicit', or the filter type of the parameter path."""
    if wkind == 'explicit':
        return scaled_inputs(name, layout, 0, 0)[2].astype(np.complex128)
    z, s, p = scaled_params(name, layout, wkind)
    return orc.effective_filter(z.astype(np.float64), s.astype(np.float64), p.astype(np.float64), wkind, dims(name)[4])


LIN_SHIFT = -200


@functools.lru_cache(maxsize=None)
def reference(name, layout, regime, wkind='explicit'):
    """(y, gx, gW) complex128 of the layout at gX = gG = 0, in the given regime -- the one oracle evaluation everything rescales."""
    edges, sten = mesh(name)[:2]
    x, gy, _ = scaled_inputs(name, layout, 0, 0)
    x, gy = x.astype(np.complex128), gy.astype(np.complex128)
    W = filter_of(name, layout, wkind)
    if regime == 'lin':
        x = x * 2.0 ** LIN_SHIFT
        assert orc.is_origin(x).all()
    else:
        box = orc.is_origin(x)
        assert box.sum() == (x == 0).sum() + 3 * special_rows(name).size       # exact zeros and the planted entries, nothing else
    y, gx, gW = orc.fieldconv_forward_backward(x, edges, sten.astype(np.complex128), W, gy)
    if regime == 'lin':
        y, gW = y * 2.0 ** -LIN_SHIFT, gW * 2.0 ** -LIN_SHIFT
    for t in (y, gx, gW):
        t.setflags(write=False)
    return y, gx, gW


def scaled_reference(name, layout, gX, gG, wkind='explicit'):
    y, gx, gW = reference(name, layout, regime_of(gX), wkind)
    return y * 2.0 ** gX, gx * 2.0 ** gG, gW * 2.0 ** (gX + gG)


def assert_reference_in_range(name, layout, gX, gG, tag='', wkind='explicit'):
    """The conditions on the inputs: every reference output is an fp32 number, and at most MAX_EXCLUDED of the rows of any tensor are
    too small to be measured."""
    y, gx, gW = scaled_reference(name, layout, gX, gG, wkind)
    yn, gxn = normalised(name, layout, y, gx)
    fmax = float(np.finfo(np.float32).max)
    for label, t, raw in (('y', yn, y), ('gx', gxn, gx), ('gW', gW, gW)):
        assert np.isfinite(raw.astype(np.complex64).view(np.float32)).all() and np.abs(raw).max() < fmax, (name, layout, tag, label)
        share = excluded_rows(t).mean()
        assert share <= MAX_EXCLUDED, (name, layout, tag, label, share)


def direct_reference(name, layout, gX, gG):
    """The oracle on the scaled inputs themselves (what scaled_reference must reproduce)."""
    edges, sten = mesh(name)[:2]
    x, gy, W = (t.astype(np.complex128) for t in scaled_inputs(name, layout, gX, gG))
    return orc.fieldconv_forward_backward(x, edges, sten.astype(np.complex128), W, gy)


def normalised(name, layout, y, gx):
    """y with column o divided by 2^b_o (y[n,o] is linear in W[o]) and gx with column i divided by 2^c_i (gx[j,i] is linear in W[:,i])."""
    _, _, b, c = exponents(name, layout)
    return np.asarray(y) * _pow2(-b)[None, :], np.asarray(gx) * _pow2(-c)[None, :]


def errors(name, layout, got, ref):
    """Row-wise errors (y, gx, gW) of got = (y, gx, gW) against ref, by the measures of the module docstring."""
    yn, gxn = normalised(name, layout, got[0], got[1])
    yr, gxr = normalised(name, layout, ref[0], ref[1])
    return measured_err(yn, yr), measured_err(gxn, gxr), measured_err(got[2], ref[2])


# ---------------------------------------------------------------- containment: a perturbed set P and who can see it
def perturbed_set(name):
    """About 1 % of the vertices: the LAST vertex of every sixth tile, so that the row that directly follows it starts the next tile
    and the rest of its own tile lies in front of it."""
    N = dims(name)[0]
    P = np.arange(TILE - 1, N - 1, 6 * TILE)
    return P[~np.isin(P, [ZERO_X_ROW, mesh(name)[2], mesh(name)[3]] + list(special_rows(name)))]


def affected_rows(name, P):
    """(y rows with an in-edge from P, gx rows with an out-edge into P or in P) as boolean masks."""
    N = dims(name)[0]
    edges = mesh(name)[0]
    inP = np.zeros(N, bool)
    inP[P] = True
    ya = np.zeros(N, bool)
    ya[edges[inP[edges[:, 0]], 1]] = True
    ga = inP.copy()
    ga[edges[inP[edges[:, 1]], 0]] = True
    return ya, ga
