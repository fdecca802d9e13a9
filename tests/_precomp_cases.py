"""Inputs and references for the per-edge tests of FCPrecomp and the support-graph build (csrc/fc_precomp.hip, csrc/fc_graph.hip;
test_precomp_host.py pins this generator on the CPU, test_gpu_precomp.py runs the kernels on it).

Supports are planted, not sampled.  The radius set planted(R, eps) holds eps * knot_q for every float32 knot sqrt(q / (R-1)) with both
float32 neighbours, 0 with both neighbours (the smallest denormals), eps with both neighbours, +inf and NaN; the angles hold 0, +-pi, the
float32 neighbours of +-float32(pi) and a few values of magnitude 50.  Further cases plant the edge counts around the 128-edge workgroups
of the builders, two workgroups that keep nothing, a support that keeps nothing, vertex areas over 40 binary orders with zero-area
sources and a target whose area sum is zero, duplicate edges, (vertex, ring) runs of 31 / 32 / 33 / 64 edges (kShortRun = 32) and more
long runs than graph_order_long_kernel has workgroups.

precomp_ref restates reference transforms/fc_precomp.py:10-27,53-97.  What rounds in float32 BY CONSTRUCTION is taken in float32 on the
CPU -- r = logMag / float32(eps) (an IEEE division on both sides: the build has no fast-math flag), the knots, the keep mask r <= 1,
the upper knot -- so kept edges and ring indices are decided by bit-identical arithmetic and compared exactly, with no exclusion mask.
Everything else is float64: ln, the area sums, wxp, the interpolation weights, e^{i m theta} and the stencil rows.

The angle m * theta exists in two forms.  The reference, the literal builder and the factored records rec_t / rec_s form the product
in float32 before sin / cos (`sten`, `ph`).  The (E,8) factor table and geo_t hold g = e^{i theta} alone and everything built from
them (FactoredStencil.materialize, the geometric-phase kernels) takes powers of g, where no product is rounded: those rows are
compared with `sten_exact`, the same rows with m * theta in float64.  The two differ by |fl32(m theta) - m theta| <= ulp(m theta) / 2,
which is 0 for |m| <= 2 and reaches 7.6e-6 at |m| = 3, |theta| = 50.

graph_ref restates the grouping: rowptr, a stable sort by (vertex, ring, edge id), the other endpoint per slot, the ring-run offsets."""
import functools
import math

import numpy as np
import torch

from oracle import torch_composites as tc

FLOOR = 1e-6                    # floor of every per-edge gate (4 x the float32 restatement's own per-edge error above it)
TINY = 1e-30                    # ln of an edge at r ~ 0 is measured against max(r, TINY)
WORKGROUP = 128                 # kPrecompEdges, kAnalyzeEdges: edges per workgroup of the builders
SHORT_RUN = 32                  # kShortRun: longer (vertex, ring) runs are ranked by graph_order_long_kernel
LONG_WORKGROUPS = 256           # ... whose 256 workgroups stride over them
PI32 = np.float32(math.pi)

# name: (band limit, rings, epsilon)
CASES = {}
for _R, _B in ((2, 2), (3, 1), (6, 2), (8, 2)):
    CASES['knots-R%d-e1' % _R] = (_B, _R, 1.0)
    CASES['knots-R%d-e03' % _R] = (_B, _R, 0.3)
CASES.update({
    'B0-R6': (0, 6, 0.3), 'B3-R8': (3, 8, 0.3),
    'literal-R12-B6': (6, 12, 0.3), 'literal-R9-B1': (1, 9, 1.0),
    'sizes-E1': (2, 6, 0.3), 'sizes-E127': (2, 6, 0.3), 'sizes-E128': (2, 6, 0.3), 'sizes-E129': (2, 6, 0.3), 'sizes-E257': (2, 6, 0.3),
    'gap': (2, 6, 0.3), 'none-kept': (2, 6, 0.3), 'areas': (2, 6, 0.3),
    'dups-i32': (2, 6, 0.3), 'dups-T': (2, 6, 0.3),
    'runs-32-33': (2, 6, 1.0), 'many-long-runs': (2, 6, 1.0),
})
LITERAL_CASES = ('literal-R12-B6', 'literal-R9-B1')
# shapes without record-driven kernels (fc_shape_compiled: R <= 8, 1 <= B <= 3): FCPrecomp hands back the dense rows
DENSE_CASES = LITERAL_CASES + ('B0-R6',)
GRAPH_CASES = tuple(n for n in CASES if n.startswith('knots')) + ('areas', 'runs-32-33', 'many-long-runs')
RUN_LENGTHS = (31, 32, 33, 64)
LONG_RUN_LENGTHS = (33, 36, 40)
AREAS_ZERO_SOURCES = (5, 6, 7)
AREAS_ZERO_TOTAL, AREAS_NO_IN, AREAS_NO_OUT = 10, 11, 12


def knots32(R):
    """The float32 knots sqrt(q / (R-1)), both operations correctly rounded as IEEE 754 asks and the device does (the float64 root of
    a float32 rounds to the correctly rounded float32 root).  torch.sqrt on a CPU need not be: builds that take the root from a
    vector library are one ulp off at sqrt(1/5) and sqrt(4/5), which moves an edge planted ON the knot into the next ring."""
    quotient = np.arange(R, dtype=np.float32) / np.float32(R - 1)
    return torch.from_numpy(np.sqrt(quotient.astype(np.float64)).astype(np.float32))


def planted_radii(R, eps):
    """float32 logMag values: eps * knot_q and both neighbours, 0 and both neighbours, eps and both neighbours, +inf, NaN"""
    e32 = np.float32(eps)
    base = [np.float32(0.0), e32] + [np.float32(e32 * k) for k in knots32(R).numpy()]
    vals = []
    for b in base:
        vals += [b, np.nextafter(b, np.float32(-np.inf)), np.nextafter(b, np.float32(np.inf))]
    return np.array(vals + [np.float32(np.inf), np.float32(np.nan)], dtype=np.float32)


def planted_angles():
    up, dn = np.float32(np.inf), np.float32(-np.inf)
    return np.array([0.0, PI32, -PI32, np.nextafter(PI32, up), np.nextafter(PI32, dn), np.nextafter(-PI32, up), np.nextafter(-PI32, dn),
                     np.float32(50.123), np.float32(-49.871), np.float32(50.0), np.float32(-47.3)], dtype=np.float32)


def ring_radii(rng, R, eps, q, n):
    """n float32 radii well inside ring q (between knots q and q+1)"""
    k = knots32(R).numpy().astype(np.float64)
    t = rng.uniform(0.1, 0.9, n)
    return ((k[q] + t * (k[q + 1] - k[q])) * eps).astype(np.float32)


def _finish(name, rng, N, src, dst, logMag, w=None, logAng=None):
    B, R, eps = CASES[name]
    E = len(src)
    if logAng is None:
        logAng = rng.uniform(-math.pi, math.pi, E).astype(np.float32)
        spec = planted_angles()
        at = rng.permutation(E)[:len(spec)]
        logAng[at] = spec[:len(at)]
    xp = np.exp(1j * rng.uniform(-math.pi, math.pi, E)).astype(np.complex64)
    if w is None:
        w = ((1.0 + 0.1 * rng.random(N)) / N).astype(np.float32)
    return dict(name=name, B=B, R=R, epsilon=eps, N=N,
                logMag=torch.from_numpy(np.asarray(logMag, dtype=np.float32).copy()), logAng=torch.from_numpy(logAng.copy()),
                xp=torch.from_numpy(xp), w=torch.from_numpy(w.copy()).reshape(N, 1),
                supp_edges=torch.from_numpy(np.stack([src, dst], 1).astype(np.int64)))


def _random_radii(rng, eps, n, outside=0.25):
    """uniform radii, a share `outside` of them beyond the support radius"""
    return (rng.uniform(0, 1, n) * eps * (1.0 / (1.0 - outside))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def case(name):
    """The inputs of FCPrecomp for one case: logMag (E), logAng (E) float32, xp (E) complex64, w (N,1) float32, supp_edges (E,2) int64,
    epsilon, N, and B, R.  Deterministic: the seed is the case's position in CASES."""
    B, R, eps = CASES[name]
    rng = np.random.default_rng(1000 + list(CASES).index(name))
    if name.startswith('knots') or name in ('B0-R6', 'B3-R8') or name in LITERAL_CASES:
        N = 40
        P = planted_radii(R, eps)
        logMag = np.concatenate([P, P, _random_radii(rng, eps, 200)])
        logMag = logMag[rng.permutation(len(logMag))]
        E = len(logMag)
        return _finish(name, rng, N, rng.integers(0, N, E), rng.integers(0, N, E), logMag)
    if name.startswith('sizes'):
        E, N = int(name[len('sizes-E'):]), 30
        logMag = _random_radii(rng, eps, E)
        logMag[0] = 0.5 * eps                                                # (E = 1: the one edge is kept)
        return _finish(name, rng, N, rng.integers(0, N, E), rng.integers(0, N, E), logMag)
    if name == 'gap':
        E, N = 3 * WORKGROUP + 2 * WORKGROUP + 37, 50
        logMag = _random_radii(rng, eps, E)
        out = rng.uniform(1.01, 3.0, 2 * WORKGROUP).astype(np.float32) * np.float32(eps)
        out[::17], out[5::31] = np.inf, np.nan
        logMag[WORKGROUP:3 * WORKGROUP] = out                                 # workgroups 1 and 2 keep nothing
        logMag[WORKGROUP - 1], logMag[3 * WORKGROUP] = 0.25 * eps, 0.75 * eps  # kept edges on both sides
        return _finish(name, rng, N, rng.integers(0, N, E), rng.integers(0, N, E), logMag)
    if name == 'none-kept':
        E, N = 200, 30
        logMag = rng.uniform(1.01, 3.0, E).astype(np.float32) * np.float32(eps)
        logMag[3], logMag[4] = np.inf, np.nan
        return _finish(name, rng, N, rng.integers(0, N, E), rng.integers(0, N, E), logMag)
    if name == 'areas':
        N, E = 64, 400
        w = np.ldexp(1.0 + 0.999 * rng.random(N), -1 - (np.arange(N) * 7 % 40)).astype(np.float32)      # 2^-40 .. 2^0
        w[list(AREAS_ZERO_SOURCES)] = 0.0
        w[0], w[1] = 1.0, 2.0 ** -40
        special = (AREAS_ZERO_TOTAL, AREAS_NO_IN, AREAS_NO_OUT)
        pool = np.array([v for v in range(N) if v not in special])
        src = rng.choice(np.append(pool, [AREAS_ZERO_TOTAL, AREAS_NO_IN]), E)
        dst = rng.choice(np.append(pool, [AREAS_NO_OUT]), E)
        logMag = _random_radii(rng, eps, E)
        # the zero-total target: in-edges from the zero-area sources only; one dropped in-edge for the vertex without in-edges and one
        # dropped out-edge for the vertex without out-edges (so that selection, not the edge list, empties them)
        zsrc = np.array(AREAS_ZERO_SOURCES + AREAS_ZERO_SOURCES[:1])
        src = np.concatenate([src, zsrc, [3, AREAS_NO_OUT]])
        dst = np.concatenate([dst, np.full(len(zsrc), AREAS_ZERO_TOTAL), [AREAS_NO_IN, 4]])
        logMag = np.concatenate([logMag, ring_radii(rng, R, eps, 2, len(zsrc)), np.float32([1.5 * eps, 2.0 * eps])])
        order = rng.permutation(len(src))
        return _finish(name, rng, N, src[order], dst[order], logMag[order], w=w)
    if name.startswith('dups'):
        N, E = 20, 150
        src, dst = rng.integers(0, N, E), rng.integers(0, N, E)
        logMag = _random_radii(rng, eps, E)
        for a, (s, d) in enumerate(((3, 7), (7, 3), (9, 9))):                # the same pair three times, in different rings
            for j in range(3):
                e = 10 + 40 * j + a
                src[e], dst[e] = s, d
                logMag[e] = ring_radii(rng, R, eps, (a + 2 * j) % (R - 1), 1)[0]
        return _finish(name, rng, N, src, dst, logMag)
    if name == 'runs-32-33':
        # target side: vertex t has RUN_LENGTHS[t] in-edges in ring t and 3 more in ring (t + 2) % 5, from a pool of sources;
        # source side: vertex 4 + t the same with out-edges into a pool of targets
        N, n_rings = 80, R - 1
        pool = np.arange(8, N)
        src, dst, mag = [], [], []
        for t, length in enumerate(RUN_LENGTHS):
            for q, n in ((t % n_rings, length), ((t + 2) % n_rings, 3)):
                others = rng.choice(pool, n, replace=True)
                src += list(others); dst += [t] * n; mag += list(ring_radii(rng, R, eps, q, n))
                others = rng.choice(pool, n, replace=True)
                src += [4 + t] * n; dst += list(others); mag += list(ring_radii(rng, R, eps, q, n))
        n_fill = 120
        src += list(rng.choice(pool, n_fill)); dst += list(rng.choice(pool, n_fill)); mag += list(_random_radii(rng, eps, n_fill))
        order = rng.permutation(len(src))
        return _finish(name, rng, N, np.array(src)[order], np.array(dst)[order], np.array(mag, dtype=np.float32)[order])
    if name == 'many-long-runs':
        # sources 160..319, targets 0..159, an edge b -> a for (b - a) mod 160 < 109: offsets 0..32 lie in ring 0, 33..68 in ring 2,
        # 69..108 in ring 4, so every target AND every source has runs of 33, 36 and 40 edges: 480 long runs per side
        half, N = 160, 320
        a, d = np.meshgrid(np.arange(half), np.arange(sum(LONG_RUN_LENGTHS)), indexing='ij')
        a, d = a.ravel(), d.ravel()
        ring = np.where(d < LONG_RUN_LENGTHS[0], 0, np.where(d < LONG_RUN_LENGTHS[0] + LONG_RUN_LENGTHS[1], 2, 4))
        mag = np.empty(len(a), dtype=np.float32)
        for q in (0, 2, 4):
            mag[ring == q] = ring_radii(rng, R, eps, q, int((ring == q).sum()))
        order = rng.permutation(len(a))
        return _finish(name, rng, N, (half + (a + d) % half)[order], a[order], mag[order])
    raise KeyError(name)


def support_data(name):
    from fieldconv_amd.data.synthetic import SupportData
    c = case(name)
    return SupportData(logMag=c['logMag'], logAng=c['logAng'], xp=c['xp'], w=c['w'], supp_edges=c['supp_edges'], epsilon=c['epsilon'],
                       num_nodes=c['N'])


def ring_index(r32, R):
    """hi - 1 for float32 radii r32 <= 1: hi is the first knot >= r, never knot 0 (float32 comparisons against the float32 knots)"""
    ge = knots32(R)[None, 1:] >= r32[:, None]
    assert bool(ge.any(1).all())
    return torch.argmax(ge.to(torch.int8), dim=1)                # (the index into knots[1:] IS hi - 1)


@functools.lru_cache(maxsize=None)
def precomp_ref(name):
    """float64 restatement of FCPrecomp on case(name); every array in kept-edge order.  keep: indices of the kept edges, edges (E',2),
    q = hi - 1, r, ln, total (N), wxp (= c), w0, w1, g = e^{i theta}, ph (E',F) = e^{i fl32(m theta)} wxp, sten (E',R,F) with that
    angle, sten_exact with m * theta in float64."""
    c = case(name)
    B, R, N = c['B'], c['R'], c['N']
    r32 = torch.from_numpy(c['logMag'].numpy() / np.float32(c['epsilon']))       # the one float32 division
    keep = torch.nonzero(r32 <= 1.0).squeeze(-1)
    r32, theta32 = r32[keep], c['logAng'][keep]
    edges, xp = c['supp_edges'][keep], c['xp'][keep].to(torch.complex128)
    q = ring_index(r32, R)
    k = knots32(R).double()
    r, theta = r32.double(), theta32.double()
    w_hi = (r - k[q]) / (k[q + 1] - k[q])
    g = torch.polar(torch.ones_like(theta), theta)
    ln = r * g
    m = torch.arange(-B, B + 1)
    ang32 = (m[None, :] * theta32[:, None])                                      # float32 product, as the reference forms it
    assert ang32.dtype == torch.float32
    freq = torch.polar(torch.ones_like(ang32, dtype=torch.float64), ang32.double())
    ang_exact = m[None, :].double() * theta[:, None]
    freq_exact = torch.polar(torch.ones_like(ang_exact), ang_exact)
    w64 = c['w'][:, 0].double()
    ws = w64[edges[:, 0]]
    total = torch.zeros(N, dtype=torch.float64).index_add(0, edges[:, 1], ws)
    wxp = (ws / (1e-12 + total[edges[:, 1]])) * xp
    ring = torch.zeros(len(keep), R, dtype=torch.float64)
    ring.scatter_(1, (q + 1)[:, None], w_hi[:, None])
    ring.scatter_(1, q[:, None], (1 - w_hi)[:, None])
    out = dict(keep=keep, edges=edges, q=q, r=r, ln=ln, total=total, wxp=wxp, w0=1 - w_hi, w1=w_hi, g=g, ph=freq * wxp[:, None],
               sten=ring[:, :, None] * freq[:, None, :] * wxp[:, None, None],
               sten_exact=ring[:, :, None] * freq_exact[:, None, :] * wxp[:, None, None])
    return {key: v.numpy() for key, v in out.items()}


def knot_neighbour(name):
    """per kept edge: its radius is one of the planted ones (on a knot, at 0, at epsilon, or one ulp to either side)"""
    c = case(name)
    return np.isin(c['logMag'].numpy()[precomp_ref(name)['keep']], planted_radii(c['R'], c['epsilon']))


@functools.lru_cache(maxsize=None)
def precomp_f32(name):
    """the float32 restatement (oracle.torch_composites.fc_precomp) on the CPU, and the per-edge quantities of the factor table in
    float32 the way it forms them: the ring weights (radial_interpolant) and g = polar(1, theta)"""
    c = case(name)
    edges, sten, ln, wxp = tc.fc_precomp(c['logMag'], c['logAng'], c['w'], c['supp_edges'], c['xp'], c['B'], c['R'], c['epsilon'])
    keep = torch.nonzero(c['logMag'] / c['epsilon'] <= 1.0).squeeze(-1)
    ring = tc.radial_interpolant((c['logMag'] / c['epsilon'])[keep], c['R'])
    q = torch.from_numpy(precomp_ref(name)['q'])
    rows = torch.arange(len(keep))
    theta = c['logAng'][keep]
    out = dict(edges=edges, sten=sten, ln=ln, wxp=wxp, ring=ring, w0=ring[rows, q], w1=ring[rows, q + 1], g=torch.polar(torch.ones_like(theta), theta))
    return {key: v.numpy() for key, v in out.items()}


def per_edge_err(got, ref, scale):
    """max over edges of max|delta_e| / scale_e; an edge with scale 0 must be exactly equal (counted as 0).  NaN anywhere fails."""
    got, ref, scale = np.asarray(got), np.asarray(ref), np.asarray(scale, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    if got.shape[0] == 0:
        return 0.0
    num = np.abs(got.reshape(got.shape[0], -1).astype(np.complex128) - ref.reshape(ref.shape[0], -1)).max(axis=1)
    assert np.all(np.isfinite(num))
    assert np.all(num[scale == 0] == 0), 'an edge whose reference is exactly zero is not'
    live = scale > 0
    return float((num[live] / scale[live]).max(initial=0.0))


def errors(name, got):
    """Per-edge errors against precomp_ref of whatever `got` holds of: ln (over max(r, TINY)), wxp and c (over |wxp_e|), sten (rows with
    fl32(m theta)) and sten_exact (rows from powers of g), both over |wxp_e|, w0 / w1 / g (absolute: their scale is 1)."""
    ref = precomp_ref(name)
    mag = np.abs(ref['wxp'])
    one = np.ones(len(mag))
    scales = dict(ln=np.maximum(ref['r'], TINY), wxp=mag, c=mag, sten=mag, sten_exact=mag, ph=mag, w0=one, w1=one, g=one)
    refs = dict(ref, c=ref['wxp'])
    return {key: per_edge_err(val, refs[key], scales[key]) for key, val in got.items()}


@functools.lru_cache(maxsize=None)
def own_errors(name):
    """the float32 restatement's per-edge errors: a gate is 4 x these, floor FLOOR.  The float32 restatement forms m * theta in
    float32, so its rows are measured against `sten`; that figure gates the rows from powers of g (against sten_exact) as well."""
    f = precomp_f32(name)
    e = errors(name, dict(ln=f['ln'], wxp=f['wxp'], sten=f['sten'], w0=f['w0'], w1=f['w1'], g=f['g']))
    e['c'], e['sten_exact'], e['ph'] = e['wxp'], e['sten'], e['sten']
    return e


def gate_of(own):
    return max(FLOOR, 4.0 * own)


def graph_ref(edges, q, N):
    """Both groupings of the edge list: side 't' groups by target (column 1), 's' by source.  rowptr (N+1) int32, perm (E) int64 = the
    stable order by (vertex, q, edge id), nbr (E) int32 = the other endpoint per slot, runs (N,8) int32 = the number of the vertex's
    edges with ring index < q."""
    edges, q = np.asarray(edges, dtype=np.int64).reshape(-1, 2), np.asarray(q, dtype=np.int64)
    out = {}
    for side, col in (('t', 1), ('s', 0)):
        v = edges[:, col]
        perm = np.lexsort((np.arange(len(v)), q, v))                   # last key first: vertex, then ring, then edge id
        hist = np.zeros((N, 8), dtype=np.int64)
        np.add.at(hist, (v, q), 1)
        rowptr = np.concatenate([[0], np.cumsum(hist.sum(1))])
        out['rowptr_' + side] = rowptr.astype(np.int32)
        out['perm_' + side] = perm.astype(np.int64)
        out['nbr_' + side] = edges[perm, 1 - col].astype(np.int32)
        out['runs_' + side] = (np.cumsum(hist, 1) - hist).astype(np.int32)
        out['hist_' + side] = hist
    return out


def record_ref(name):
    """the edge-order factored records of precomp_ref(name) in float64: (E', 4 + 2F) [q, w0, w1, 0, Re / Im ph_f ...] (q as a number)"""
    ref = precomp_ref(name)
    E, F = ref['ph'].shape
    rec = np.zeros((E, 4 + 2 * F))
    rec[:, 0], rec[:, 1], rec[:, 2] = ref['q'], ref['w0'], ref['w1']
    rec[:, 4::2], rec[:, 5::2] = ref['ph'].real, ref['ph'].imag
    return rec


def row_exponents(name, lo=-70, hi=20):
    """per kept edge, the exponent s of the factor 2^s of the row-scaling test"""
    n = len(precomp_ref(name)['keep'])
    return np.random.default_rng(77).integers(lo, hi + 1, n)
