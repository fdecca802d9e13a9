"""Inputs and references for the row-by-row tests of the TransField and ECHO descriptor kernels (test_lift_echo_host.py pins this
generator on the CPU; test_gpu_lift_echo.py runs the kernels on it).

Meshes are planted, not sampled: the in-degrees that the prefetch groups, the wavefronts-per-vertex merge and the partly filled
workgroups turn on are put there by hand (MESHES, planted_degrees), and the total edge count puts E // N on the chosen side of the
wavefront thresholds.  The references are oracle.torch_composites.trans_field / echo_descriptors on the CPU, in float64 / complex128
(the reference proper) and in float32 / complex64 (the float32 restatement whose own row-wise error, times 4, is the gate).

Rows are scaled by POWERS OF TWO that are exact in the reference:

    TransField: the stencil rows of all in-edges of target n times 2^a_n  ->  y[n,:] times exactly 2^a_n
                (mag is linear in |s0|, angle(A) does not see a positive factor)
    ECHO:       wxp of the in-edges of n times 2^a_n                      ->  desc[n] times exactly 2^a_n
                (the votes depend on ln and the frame only)

with two provisos, both absolute 1e-7 bounds (the origin box): a stencil entry, an A = sum_r ang zonalAng or a histogram entry must
not cross the box when its row is scaled.  Stencil entries are exact zeros or far outside at every exponent; no A may have its larger
component in [1e-8, 1e-6] (asserted); histogram entries near that range are left out under a cap (see echo_masks)."""
import functools

import numpy as np
import torch

from _dynamic_range_cases import MAX_EXCLUDED, excluded_rows, measured_err, rowwise_err      # noqa: F401  (the measure: imported, not copied)
from oracle import torch_composites as tc

WPG = 4                         # wavefronts per workgroup = vertices per workgroup at one wavefront per vertex (kTfWaves, kEchoWaves)
TF_AHEAD, ECHO_AHEAD = 8, 4     # kTfAhead, kEchoAhead: edges per prefetch group
TF_RANGE = (-8, 8)              # exponents of the stencil rows
ECHO_RANGE = (-8, 8)            # exponents of the wxp rows
LAYOUTS = ('random', 'groups')
BOX_LO, BOX_HI = 1e-8, 1e-6     # a factor of 10 on either side of the 1e-7 origin-box bound
FRAGILE = 1e-5                  # a vote coordinate this close to a raster line is fragile
MAX_FRAGILE = 1e-2              # share of descriptor entries left out for fragile votes and near-box histogram entries
PERTURB_EXP = 40
FLOOR = 1e-6                    # floor of the float32 gates
F64_GATE = 1e-12


def waves_per_vertex(N, E):
    """Wavefronts that share a vertex: tf_waves_per_vertex (csrc/fc_trans_field.hip) and echo_waves_per_vertex (csrc/fc_echo.hip; without
    FC_ECHO_WPV) -- the same rule in both, restated here once."""
    deg = E // N if N > 0 else 0
    if deg >= 64 and N < 65536:
        return 4
    if deg >= 32 and N < 131072:
        return 2
    return 1


def planted_degrees(wpv, ahead):
    """Row lengths at the edges of the prefetch loop (`ahead` edges per wavefront and round, every wpv-th edge to a wavefront): empty,
    shorter than / exactly one edge per wavefront, one short of / exactly / one over one prefetch group, two groups, two groups and one."""
    g = ahead * wpv
    return [0, 1, wpv - 1, wpv, g - 1, g, g + 1, 2 * g, 2 * g + 1]


# name: (N, E // N, planted row lengths, quiet perturbed set)
MESHES = {
    'w1-31': (45, 31, True, False),             # one wavefront per vertex, just below the threshold; N % 4 = 1
    'w2-32': (45, 32, True, False),             # two, just above; odd N: the last workgroup holds one vertex
    'w2-63': (81, 63, True, False),             # two, just below the next threshold; odd N
    'w4-64': (83, 64, True, False),             # four
    'n42': (42, 6, True, False),                # N % 4 = 2
    'n43': (43, 6, True, False),                # N % 4 = 3
    'n1': (1, 1, False, False),                 # one vertex, one self-edge
    'quiet1': (403, 5, False, True),            # containment, one wavefront per vertex
    'quiet2': (203, 32, False, True),           # containment, two wavefronts per vertex: the LDS merge
    'plan37': (37, 4, False, False),            # TransField backward: 12 persistent wavefronts, not a multiple of the 16 reduction ways
    'plan4095': (4095, 4, False, False),        # ... a quarter of the vertices, rounded up to whole workgroups: 1024
    'plan4099': (4099, 4, False, False),        # ... the fixed 1024 (N >= 4096)
}


def perturbed_set(N):
    """The LAST vertex of every sixth workgroup (as _dynamic_range_cases.perturbed_set: its successor starts the next workgroup)."""
    return np.arange(WPG - 1, N - 1, 6 * WPG)


@functools.lru_cache(maxsize=None)
def mesh(name, ahead):
    """(edges (E,2) int64 [source, target] in shuffled order, the vertex without out-edges or None).  In a quiet mesh the vertices of
    perturbed_set have 3 in-edges and 2 out-edges, so that most rows cannot see them."""
    N, D, planted, quiet = MESHES[name]
    if N == 1:
        return np.zeros((1, 2), np.int64), None
    rng = np.random.default_rng([N, D, ahead])
    E = D * N + N // 2
    wpv = waves_per_vertex(N, E)
    P = perturbed_set(N) if quiet else np.zeros(0, np.int64)
    no_out = N // 2 + 1
    assert no_out not in P
    deg = np.full(N, -1)
    deg[P] = 3
    free = np.array([v for v in rng.permutation(N) if v not in P])
    if planted:
        pd = planted_degrees(wpv, ahead)
        deg[free[:len(pd)]] = pd
    rest = np.flatnonzero(deg < 0)
    left = E - int(deg[deg >= 0].sum())
    deg[rest] = left // rest.size + (np.arange(rest.size) < left % rest.size)
    banned = np.zeros(N, bool)
    banned[P] = True
    banned[no_out] = True
    src, dst = [], []
    for n in range(N):
        pool = np.flatnonzero(~banned & (np.arange(N) != n))
        src.append(rng.choice(pool, deg[n], replace=deg[n] > pool.size))
        dst.append(np.full(deg[n], n))
    src, dst = np.concatenate(src), np.concatenate(dst)
    if quiet:               # two out-edges per perturbed vertex, into ordinary vertices
        slots = rng.choice(np.flatnonzero(~np.isin(dst, P)), 2 * P.size, replace=False)
        src[slots] = np.repeat(P, 2)
    order = rng.permutation(E)
    edges = np.stack((src[order], dst[order]), 1).astype(np.int64)
    assert edges.shape[0] == E and E // N == D and not (edges[:, 0] == no_out).any()
    edges.setflags(write=False)
    return edges, no_out


def in_degrees(name, ahead):
    return np.bincount(mesh(name, ahead)[0][:, 1], minlength=MESHES[name][0])


@functools.lru_cache(maxsize=None)
def exponents(N, layout, lo, hi):
    """One exponent per vertex.  'random': every 4-vertex workgroup spans [lo, hi] and the last vertex is pinned to lo; 'groups': whole
    workgroups alternate between hi and lo."""
    rng = np.random.default_rng([N, LAYOUTS.index(layout)])
    if layout == 'random':
        a = rng.integers(lo, hi + 1, N)
        a[0::WPG] = hi
        a[WPG - 1::WPG] = lo
        a[N - 1] = lo
    else:
        a = np.where((np.arange(N) // WPG) % 2 == 0, hi, lo)
    a.setflags(write=False)
    return a


def _pow2(e):
    return np.ldexp(1.0, np.asarray(e))


def _away_from_zero(rng, shape, floor):
    """N(0,1) with |value| >= floor"""
    v = rng.standard_normal(shape)
    return np.where(np.abs(v) < floor, np.where(v < 0, -floor, floor), v)


def affected_rows(edges, N, P):
    """(rows in P or with an in-edge from P, rows in P or with an out-edge into P) as boolean masks"""
    inP = np.zeros(N, bool)
    inP[P] = True
    fwd, bwd = inP.copy(), inP.copy()
    fwd[edges[inP[edges[:, 0]], 1]] = True
    bwd[edges[inP[edges[:, 1]], 0]] = True
    return fwd, bwd


# ---------------------------------------------------------------------------------------------- TransField
# name: (mesh, Cin, R, O, ftype, layout, float64)
TF_CASES = {}
for _m in ('w1-31', 'w2-32', 'w2-63', 'w4-64', 'n42', 'n43', 'n1'):          # row lengths, wavefronts per vertex, partly filled workgroups
    TF_CASES['rows-' + _m] = (_m, 3, 6, 48, 1, 'random', False)
for _m in ('w1-31', 'w2-32'):
    TF_CASES['rows-' + _m + '-groups'] = (_m, 3, 6, 48, 1, 'groups', False)
TF_SPECIALISED_SIZES = ((4, 8, 64), (1, 1, 1), (3, 6, 48))                   # at the lane limits
TF_GENERIC_SIZES = ((5, 6, 16), (3, 9, 16), (3, 6, 65))                      # just outside: the run-time kernels
for _s in TF_SPECIALISED_SIZES + TF_GENERIC_SIZES:
    for _ft in (0, 1):
        TF_CASES['size-%d-%d-%d-t%d' % (_s + (_ft,))] = ('n42',) + _s + (_ft, 'random', False)
TF_CASES['f64'] = ('n43', 3, 6, 48, 1, 'random', True)
for _m in ('plan37', 'plan4095', 'plan4099'):                                 # backward plan: k = 4 edges per vertex, O = 16
    TF_CASES[_m] = (_m, 3, 6, 16, 1, 'random' if _m != 'plan4095' else 'groups', False)
TF_FORM_CASES = ('rows-w1-31', 'rows-w2-32', 'rows-w2-63', 'rows-w4-64')      # packed, strided (B = 2, 3) and factor table on one mesh
TF_CONTAINMENT = {'contain-quiet1': ('quiet1', 3, 6, 48, 1, 'random', False), 'contain-quiet2': ('quiet2', 3, 6, 48, 1, 'random', False)}
TF_OUTPUTS = ('y', 'gx', 'g_zonalAng', 'g_zonalMag', 'g_phase')
# Seeds of the cases whose first draw put an A next to the origin box, or so close to zero that d angle(A) ~ 1/|A| took the float32
# restatement's gradients beyond 1e-4 (a vertex with one in-edge has A = (x_src - x_n) s1 . zonalAng: one direction, so it cancels easily)
TF_SEEDS = {'rows-w2-63': 2, 'rows-w4-64': 1, 'rows-n42': 1, 'rows-w2-32-groups': 5, 'size-3-6-48-t1': 1, 'size-5-6-16-t0': 3, 'size-5-6-16-t1': 1,
            'size-3-9-16-t1': 1, 'size-3-6-65-t1': 1, 'plan4095': 4, 'plan4099': 12}
# the cases that carry a planted exactly-zero magnitude (zero_magnitude_entry): lane-mapped kernels, run-time kernels, run-time float64
ZERO_MAGNITUDE_CASES = ('size-4-8-64-t1', 'size-3-6-65-t0', 'f64')


def tf_case(name):
    return TF_CASES[name] if name in TF_CASES else TF_CONTAINMENT[name]


def tf_specialised(Cin, R, O, f64):
    return not f64 and Cin <= 4 and R <= 8 and O <= 64


@functools.lru_cache(maxsize=None)
def tf_base(name):
    """The unscaled problem.  The stencil is FCPrecomp's factor table [q, w_q, w_{q+1}, 0, Re c, Im c, cos t, sin t] (float32; None for
    one ring) and the two columns s0 = w_r c, s1 = w_r c e^{it} that it stands for, complex64: two rings per edge carry weight, every
    seventh edge only one, the other entries are exact zeros (inside the origin box at every exponent)."""
    m, Cin, R, O, ftype, layout, f64 = tf_case(name)
    edges = mesh(m, TF_AHEAD)[0]
    N, E = MESHES[m][0], edges.shape[0]
    rng = np.random.default_rng([N, E, Cin, R, O, ftype, TF_SEEDS.get(name, 0)])
    c = (0.2 * (_away_from_zero(rng, E, 0.25) + 1j * _away_from_zero(rng, E, 0.25))).astype(np.complex64)
    t = rng.uniform(-np.pi, np.pi, E)
    g = (np.cos(t).astype(np.float32) + 1j * np.sin(t).astype(np.float32)).astype(np.complex64)
    ring = np.zeros((E, R), np.float32)
    if R == 1:
        factors = None
        ring[:, 0] = 1
    else:
        q = rng.integers(0, R - 1, E)
        w = (rng.integers(2, 15, E) / 16).astype(np.float32)
        w[::7] = 1
        ring[np.arange(E), q], ring[np.arange(E), q + 1] = w, 1 - w
        factors = np.zeros((E, 8), np.float32)
        factors[:, 0] = q.astype(np.int32).view(np.float32)
        factors[:, 1], factors[:, 2] = w, 1 - w
        factors[:, 4], factors[:, 5], factors[:, 6], factors[:, 7] = c.real, c.imag, g.real, g.imag
    s0 = ring.astype(np.float64) * c.astype(np.complex128)[:, None]
    s01 = np.stack((s0, s0 * g.astype(np.complex128)[:, None]), 2).astype(np.complex64)
    x = rng.standard_normal((N, Cin)).astype(np.float32)
    x[rng.random((N, Cin)) < 0.03] = 0
    zm = zero_magnitude_entry(name)
    if zm is not None:          # every in-neighbour of vertex n carries x = 0 in channel i: mag[n,i,:] and M[n,:,i] are exactly zero
        n, i = zm
        x[edges[edges[:, 1] == n, 0], i] = 0
        if x[n, i] == 0:
            x[n, i] = 0.5       # (the angular sums of n stay alive)
    gy = (rng.standard_normal((N, O)) + 1j * rng.standard_normal((N, O))).astype(np.complex64)
    zA, zM = (rng.uniform(-0.5, 0.5, (O, Cin, R)).astype(np.float32) for _ in range(2))
    phase = rng.uniform(-np.pi, np.pi, (O, Cin)).astype(np.float32) if ftype else np.zeros((O, Cin), np.float32)
    return dict(edges=edges, factors=factors, s01=s01, x=x, gy=gy, zonalAng=zA, zonalMag=zM, phase=phase)


def zero_magnitude_entry(name):
    """(n, i): the vertex with the fewest (but some) in-edges, and the last input channel.  tf_base zeroes x[., i] of all its
    in-neighbours, so that M[n,o,i] = sum_r mag[n,i,r] zonalMag[o,i,r] is EXACTLY zero: rho = |M| = 0, where torch.polar -- and with it the
    reference -- passes no gradient to the magnitude.  None outside ZERO_MAGNITUDE_CASES."""
    if name not in ZERO_MAGNITUDE_CASES:
        return None
    m, Cin = tf_case(name)[0], tf_case(name)[1]
    deg = in_degrees(m, TF_AHEAD)
    return int(np.flatnonzero(deg == deg[deg > 0].min())[0]), Cin - 1


def tf_exponents(name):
    m, layout = tf_case(name)[0], tf_case(name)[5]
    return exponents(MESHES[m][0], layout, *TF_RANGE)


@functools.lru_cache(maxsize=None)
def tf_problem(name, scaled=True):
    """tf_base with the stencil rows of the in-edges of n times 2^a_n (in the factor table: c); products formed in double precision."""
    p = dict(tf_base(name))
    if scaled:
        f = _pow2(tf_exponents(name))[p['edges'][:, 1]]
        p['s01'] = (p['s01'].astype(np.complex128) * f[:, None, None]).astype(np.complex64)
        if p['factors'] is not None:
            fac = p['factors'].astype(np.float64)
            fac[:, 4:6] *= f[:, None]
            fac = fac.astype(np.float32)
            fac[:, 0] = p['factors'][:, 0]          # (the ring index is an integer's bit pattern)
            p['factors'] = fac
    for v in p.values():
        if v is not None:
            v.setflags(write=False)
    return p


def _tf_run(p, real, ftype, x=None, gy=None):
    cplx = torch.complex128 if real == torch.float64 else torch.complex64
    T = lambda a, dt: torch.from_numpy(np.array(a)).to(dt)
    xt = T(p['x'] if x is None else x, real).requires_grad_(True)
    par = [T(p[k], real).requires_grad_(True) for k in ('zonalAng', 'zonalMag', 'phase')]
    y = tc.trans_field(xt, torch.from_numpy(np.array(p['edges'])), T(p['s01'], cplx), par[0], par[1], par[2], ftype)
    wrt = [xt] + par[:3 if ftype else 2]
    grads = torch.autograd.grad(y, wrt, grad_outputs=T(p['gy'] if gy is None else gy, cplx))
    out = dict(zip(TF_OUTPUTS, [y.detach().numpy()] + [g.numpy() for g in grads]))
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def tf_reference(name, precision='f64', scaled=True):
    """{y, gx, g_zonalAng, g_zonalMag (, g_phase)} of the case: the oracle's torch restatement on the CPU in float64, or in float32"""
    return _tf_run(tf_problem(name, scaled), torch.float64 if precision == 'f64' else torch.float32, tf_case(name)[4])


@functools.lru_cache(maxsize=None)
def tf_A(name):
    """The float64 A[n,o,i] = sum_r ang[n,i,r] zonalAng[o,i,r] whose angle the operator takes"""
    p = tf_problem(name)
    src, dst = p['edges'][:, 0], p['edges'][:, 1]
    x, s1 = p['x'].astype(np.float64), p['s01'][:, :, 1].astype(np.complex128)
    ang = np.zeros((x.shape[0], x.shape[1], s1.shape[1]), np.complex128)
    np.add.at(ang, dst, (x[src] - x[dst])[:, :, None] * s1[:, None, :])
    return np.einsum('nir,oir->noi', -ang, p['zonalAng'].astype(np.float64))


def near_box(z):
    """Entries whose larger component lies in [BOX_LO, BOX_HI]"""
    big = np.maximum(np.abs(z.real), np.abs(z.imag))
    return (big >= BOX_LO) & (big <= BOX_HI)


def gate_of(own_err, f64=False):
    return F64_GATE if f64 else max(4 * own_err, FLOOR)


# ---------------------------------------------------------------------------------------------- ECHO
def hist_dim(n_bins):
    return tc.disk_map(n_bins)[1]


def channel_block(n_bins):
    """fc_echo_channel_block (csrc/fc_echo.hip): the channels whose histograms of one workgroup fit into 160 KiB of LDS beside the
    raster map, at most one per lane"""
    return min(64, (160 * 1024 // 4 - 17 * 17 - 3) // (WPG * hist_dim(n_bins) * 2))


# name: (mesh, C, n_bins, layout, complex128)
ECHO_CASES = {}
for _m in ('w1-31', 'w2-32', 'w2-63', 'w4-64', 'n42', 'n43', 'n1'):
    ECHO_CASES['rows-' + _m] = (_m, 33, 2, 'random', False)
for _m in ('w1-31', 'w2-32'):
    ECHO_CASES['rows-' + _m + '-groups'] = (_m, 33, 2, 'groups', False)
for _nb in (1, 3, 5, 8):            # forward blocks of channel_block(n_bins) channels, backward blocks of 64
    for _c in sorted({channel_block(_nb), channel_block(_nb) + 1, 64, 65}):
        ECHO_CASES['blocks-b%d-c%d' % (_nb, _c)] = ('n42', _c, _nb, 'random', False)
ECHO_CASES['bins9'] = ('n42', 9, 9, 'random', False)           # n_bins > 8: the run-time kernels
ECHO_CASES['c128'] = ('n43', 17, 3, 'random', True)
ECHO_CONTAINMENT = {'contain-quiet1': ('quiet1', 33, 2, 'random', False), 'contain-quiet2': ('quiet2', 33, 2, 'random', False)}
ZERO_X_ROW = 5


def echo_case(name):
    return ECHO_CASES[name] if name in ECHO_CASES else ECHO_CONTAINMENT[name]


def echo_exponents(name):
    m, layout = echo_case(name)[0], echo_case(name)[3]
    return exponents(MESHES[m][0], layout, *ECHO_RANGE)


@functools.lru_cache(maxsize=None)
def echo_problem(name, scaled=True):
    """edges, ln (inside the unit disk, every ninth edge at its centre), wxp (times 2^a of its target when scaled), features with 5 %
    exact zeros and one all-zero row, and the gradient arriving at the descriptors"""
    m, C, n_bins, layout, c128 = echo_case(name)
    edges = mesh(m, ECHO_AHEAD)[0]
    N, E = MESHES[m][0], edges.shape[0]
    rng = np.random.default_rng([N, E, C, n_bins])
    ln = (0.98 * np.sqrt(rng.random(E)) * np.exp(1j * rng.uniform(-np.pi, np.pi, E))).astype(np.complex64)
    ln[::9] = 0
    wxp = (rng.uniform(0.5, 1.5, E) * np.exp(1j * rng.uniform(-np.pi, np.pi, E))).astype(np.complex64)
    if scaled:
        wxp = (wxp.astype(np.complex128) * _pow2(echo_exponents(name))[edges[:, 1]]).astype(np.complex64)
    x = (rng.standard_normal((N, C)) + 1j * rng.standard_normal((N, C))).astype(np.complex64)
    x[rng.random((N, C)) < 0.05] = 0
    if N > ZERO_X_ROW:
        x[ZERO_X_ROW] = 0
    gd = rng.standard_normal((N, C, hist_dim(n_bins))).astype(np.float32)
    p = dict(edges=edges, ln=ln, wxp=wxp, x=x, gd=gd)
    for v in p.values():
        v.setflags(write=False)
    return p


def _echo_run(p, n_bins, cplx, x=None, gd=None):
    real = torch.float64 if cplx == torch.complex128 else torch.float32
    T = lambda a, dt: torch.from_numpy(np.array(a)).to(dt)
    xt = T(p['x'] if x is None else x, cplx).requires_grad_(True)
    desc = tc.echo_descriptors(xt, torch.from_numpy(np.array(p['edges'])), T(p['ln'], cplx), T(p['wxp'], cplx), n_bins)
    gx, = torch.autograd.grad(desc, [xt], grad_outputs=T(p['gd'] if gd is None else gd, real))
    out = dict(desc=desc.detach().numpy(), gx=gx.numpy())
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def echo_reference(name, precision='f64', scaled=True):
    return _echo_run(echo_problem(name, scaled), echo_case(name)[2], torch.complex128 if precision == 'f64' else torch.complex64)


def fragile_votes(x, edges, ln, n_bins):
    """(fragile (N,C), tainted (N,)) boolean tensors.  The reference's votes vanish at exactly integer raster coordinates (ceil == floor,
    nn/echo.py:30-61): a coordinate that rounds to an integer in fp32 but sits 1e-7 beside it in float64 drops a whole vote.  A descriptor
    (n, c) fed by a vote with a coordinate within FRAGILE of a raster line is fragile; a vertex with an edge into a vertex that has a
    fragile channel is tainted in its gradient.  x, ln: complex128 tensors (ln as the kernels get it); edges (E,2)."""
    N, C = x.shape
    frame = torch.conj(torch.polar(torch.ones(N, C, dtype=torch.float64), torch.angle(x)))
    qq = torch.view_as_real(ln[:, None] * frame[edges[:, 0]] * n_bins)
    near = ((qq - torch.round(qq)).abs() < FRAGILE).any(dim=2) & (ln.abs() > 0)[:, None]
    cols = torch.arange(C)[None, :].expand(edges.shape[0], -1)
    fragile = torch.zeros(N, C, dtype=torch.bool)
    fragile[edges[:, 1][:, None].expand(-1, C)[near], cols[near]] = True
    tainted = torch.zeros(N, dtype=torch.bool)
    tainted[edges[:, 0][fragile.any(dim=1)[edges[:, 1]]]] = True
    return fragile, tainted


@functools.lru_cache(maxsize=None)
def echo_masks(name):
    """(ok_desc (N,C,dS), ok_gx (N,C), excluded share of desc): what is compared.  Left out are the descriptors (n, c) with a fragile vote,
    the descriptor entries whose float64 histogram entry may have its larger component in [BOX_LO, BOX_HI] -- |hist| in
    [BOX_LO, sqrt(2) BOX_HI], a superset read off the descriptor itself -- and, in the gradient, channel c of every vertex with an
    edge that votes into such an entry."""
    p, n_bins = echo_problem(name), echo_case(name)[2]
    T = lambda a: torch.from_numpy(np.array(a)).to(torch.complex128)
    edges = np.array(p['edges'])
    fragile = fragile_votes(T(p['x']), torch.from_numpy(edges), T(p['ln']), n_bins)[0].numpy()
    desc = echo_reference(name)['desc']
    box = (desc >= BOX_LO) & (desc <= BOX_HI * np.sqrt(2.0))
    bad = fragile[:, :, None] | box
    # the four bins every (edge, channel) votes into, by the oracle's own raster
    frame = torch.conj(torch.polar(torch.ones(p['x'].shape, dtype=torch.float64), torch.angle(T(p['x']))))
    ind = tc.rasterize(T(p['ln'])[:, None] * frame[edges[:, 0]], tc.disk_map(n_bins)[0], n_bins)[1].numpy()
    hit = np.take_along_axis(bad[edges[:, 1]], ind, axis=2).any(axis=2)          # (E, C)
    taint = np.zeros(p['x'].shape, bool)
    np.logical_or.at(taint, edges[:, 0], hit)
    return ~bad, ~taint, float(bad.mean())


def echo_errors(name, got, ref):
    """row-wise errors (desc, gx) over what echo_masks keeps"""
    ok, okg, _ = echo_masks(name)
    return (measured_err(np.asarray(got['desc']) * ok, ref['desc'] * ok), measured_err(np.asarray(got['gx']) * okg, ref['gx'] * okg))


def tf_errors(got, ref):
    """row-wise errors of every output.  With ONE ring g_zonalAng is left out: angle(A) does not see the length of zonalAng, so the
    gradient along zonalAng is zero, and with one ring there is no other direction -- both sides hold rounding noise only."""
    one_ring = ref['g_zonalAng'].shape[2] == 1
    return {k: measured_err(got[k], ref[k]) for k in ref if not (one_ring and k == 'g_zonalAng')}
