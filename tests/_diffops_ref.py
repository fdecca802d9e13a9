"""numpy restatement of fieldconv_amd.diffops (csrc/fc_diffops.hip): the two CSRs of a plan, the least-squares coefficients with
diag and valid, the gradient, its adjoint, the divergence and the Laplacian.  Every function takes `real`: np.float32 restates
the kernels' arithmetic, every operation rounded on its own in their order (only cos and sin are numpy's, not the device
library's); np.float64 is the yardstick of both, computed from the same float32 inputs.  Also the shared cases: the planted CSR
of the device tests and the meshes with exact log maps of the host tests.  Uses nothing from the package."""
import functools

import numpy as np

F32 = np.float32
COMPLEX = {np.dtype(np.float32): np.complex64, np.dtype(np.float64): np.complex128}
RCOND = 1e-4
LANES = 64


# ------------------------------------------------------------------ the plan's two CSRs
def csr(rows, n):
    """(by_query, rowptr, col, by_nbr, rowptr_t, col_t): slots are the rows grouped by query with a stable sort; the transposed
    slots are the slots grouped by neighbour with a second stable sort (transposed slot t is slot by_nbr[t])"""
    by_query = np.argsort(rows[:, 0], kind='stable')
    query, col = rows[by_query, 0], rows[by_query, 1]
    by_nbr = np.argsort(col, kind='stable')
    ends = np.arange(n + 1)
    return (by_query, np.searchsorted(query, ends).astype(np.int32), col.astype(np.int32), by_nbr,
            np.searchsorted(col[by_nbr], ends).astype(np.int32), query[by_nbr].astype(np.int32))


# ------------------------------------------------------------------ coefficients
def _fold(terms, where, real):
    """the kernel's order: lane l adds the terms of the slots l, l + 64, ... of its row (the active ones: `where`) to a zero in
    ascending order, then the 64 partial sums are folded p[l] += p[l + 32], ..., p[0] += p[1]"""
    p = np.zeros(LANES, dtype=real)
    for j in range(len(terms)):
        if where[j]:
            p[j % LANES] = p[j % LANES] + terms[j]
    off = LANES // 2
    while off >= 1:
        p = p[:off] + p[off:2 * off]
        off //= 2
    assert p.dtype == real
    return p[0]


def coefficients(rowptr, col, mag, ang, w, n, rcond, real):
    """(coef (E,) complex, diag (n,) complex, valid (n,) uint8, ratio (n,) det / tr^2 in `real`; NaN for an empty sum) from the
    float32 slot arrays.  In float32 the products m cos(theta), m sin(theta) are float32 products of float32 values."""
    E = len(col)
    m, th = mag.astype(real), ang.astype(real)
    in_range = (col >= 0) & (col < n)
    omega = np.ones(E, dtype=real) if w is None else np.where(in_range, w.astype(real)[np.clip(col, 0, max(n - 1, 0))], real(0))
    with np.errstate(invalid='ignore'):
        active = in_range & (m > 0) & np.isfinite(m) & np.isfinite(th) & (omega > 0) & np.isfinite(omega)
    safe_th = np.where(active, th, real(0))
    p, q = np.where(active, m * np.cos(safe_th), real(0)), np.where(active, m * np.sin(safe_th), real(0))
    assert p.dtype == real and q.dtype == real
    kr, ki = np.zeros(E, dtype=real), np.zeros(E, dtype=real)
    dr, di = np.zeros(n, dtype=real), np.zeros(n, dtype=real)
    valid, ratio = np.zeros(n, dtype=np.uint8), np.full(n, np.nan, dtype=real)
    rc = real(F32(rcond))          # rounded once to float32 by the entry point
    for a in range(n):
        s = slice(rowptr[a], rowptr[a + 1])
        P, Q, O, act = p[s], q[s], omega[s], active[s]
        op, oq = O * P, O * Q
        a11, a12, a22 = _fold(op * P, act, real), _fold(op * Q, act, real), _fold(oq * Q, act, real)
        det = a11 * a22 - a12 * a12
        tr = a11 + a22
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio[a] = det / (tr * tr)
        if not det > (rc * tr) * tr:
            continue
        valid[a] = 1
        f = O / det
        re, im = f * (a22 * P - a12 * Q), f * (a11 * Q - a12 * P)
        kr[s], ki[s] = np.where(act, re, real(0)), np.where(act, im, real(0))
        dr[a], di[a] = _fold(kr[s], act, real), _fold(ki[s], act, real)
    cplx = COMPLEX[np.dtype(real)]
    return (kr + 1j * ki).astype(cplx), (dr + 1j * di).astype(cplx), valid, ratio


# ------------------------------------------------------------------ the operators
def apply(rowptr, col, coef, x, real):
    """y[a] = sum_e coef[e] * (x[col[e]] - x[a]) in the arithmetic of `real`: the difference, the two products and the two
    additions each rounded, a row's terms added to a zero in slot order"""
    n = len(rowptr) - 1
    xs = x.astype(real)
    kr, ki = coef.real.astype(real), coef.imag.astype(real)
    yr, yi = np.zeros((n, x.shape[1]), dtype=real), np.zeros((n, x.shape[1]), dtype=real)
    for a in range(n):
        for e in range(rowptr[a], rowptr[a + 1]):
            d = xs[col[e]] - xs[a]
            yr[a] = yr[a] + kr[e] * d
            yi[a] = yi[a] + ki[e] * d
    assert yr.dtype == real
    return (yr + 1j * yi).astype(COMPLEX[np.dtype(real)])


def adjoint(rowptr_t, col_t, coef_t, diag, g, real, scale_in=None, scale_out=None):
    """gx[i] = so[i] * ((sum_t Re(conj(coef_t[t]) si[col_t[t]] g[col_t[t]])) - Re(conj(diag[i]) si[i] g[i])) on the transposed CSR, the
    t sum added to a zero in slot order"""
    n = len(rowptr_t) - 1
    gr, gi = g.real.astype(real), g.imag.astype(real)
    if scale_in is not None:
        gr, gi = scale_in.astype(real)[:, None] * gr, scale_in.astype(real)[:, None] * gi
    kr, ki = coef_t.real.astype(real), coef_t.imag.astype(real)
    dr, di = diag.real.astype(real), diag.imag.astype(real)
    out = np.zeros((n, g.shape[1]), dtype=real)
    for i in range(n):
        for t in range(rowptr_t[i], rowptr_t[i + 1]):
            out[i] = out[i] + (kr[t] * gr[col_t[t]] + ki[t] * gi[col_t[t]])
        out[i] = out[i] - (dr[i] * gr[i] + di[i] * gi[i])
    if scale_out is not None:
        out = scale_out.astype(real)[:, None] * out
    assert out.dtype == real
    return out


def scales(w, n, real):
    """(scale_in, scale_out) of the divergence: w (None without weights) and -1 / w, 0 where w == 0 (-1 without weights)"""
    if w is None:
        return None, np.full(n, -1, dtype=real)
    s = w.astype(real)
    with np.errstate(divide='ignore'):
        return s, np.where(s == 0, real(0), real(-1) / s)


class Plan:
    """the restated plan of a set of rows; coefficients in float32 and float64, or given (the device's) through `coef`"""

    def __init__(self, rows, mag, ang, n, w=None, rcond=RCOND):
        self.n, self.w, self.rcond = n, w, rcond
        self.by_query, self.rowptr, self.col, self.by_nbr, self.rowptr_t, self.col_t = csr(rows, n)
        self.mag, self.ang = mag[self.by_query], ang[self.by_query]

    @functools.lru_cache(maxsize=None)
    def coefficients(self, real):
        return coefficients(self.rowptr, self.col, self.mag, self.ang, self.w, self.n, self.rcond, real)

    def _operands(self, real, coef, diag):
        if coef is None:
            coef, diag = self.coefficients(real)[:2]
        cplx = COMPLEX[np.dtype(real)]
        return coef.astype(cplx), diag.astype(cplx)

    def gradient(self, x, real, coef=None, diag=None):
        return apply(self.rowptr, self.col, self._operands(real, coef, diag)[0], x, real)

    def gradient_adjoint(self, g, real, coef=None, diag=None):
        coef, diag = self._operands(real, coef, diag)
        return adjoint(self.rowptr_t, self.col_t, coef[self.by_nbr], diag, g, real)

    def divergence(self, v, real, coef=None, diag=None):
        coef, diag = self._operands(real, coef, diag)
        si, so = scales(self.w, self.n, real)
        return adjoint(self.rowptr_t, self.col_t, coef[self.by_nbr], diag, v, real, si, so)

    def divergence_adjoint(self, g, real, coef=None, diag=None):
        """the gradient of <g, div v> to v: S_in G (S_out g)"""
        si, so = scales(self.w, self.n, real)
        y = self.gradient(so[:, None] * g.astype(real), real, coef, diag)
        if si is None:
            return y
        return (si[:, None] * y.real + 1j * (si[:, None] * y.imag)).astype(COMPLEX[np.dtype(real)])

    def laplacian(self, f, real, coef=None, diag=None):
        return self.divergence(self.gradient(f, real, coef, diag), real, coef, diag)

    def laplacian_adjoint(self, g, real, coef=None, diag=None):
        return self.gradient_adjoint(self.divergence_adjoint(g, real, coef, diag), real, coef, diag)


# ------------------------------------------------------------------ the planted CSR of the device tests
N_PLANTED = 70
ROW_LENGTHS = {0: 0, 1: 1, 2: 2, 3: 2, 4: 3, 5: 63, 6: 64, 7: 65, 8: 129}          # row 2: collinear, row 3: independent
ZERO_WEIGHT = (13, 27)


@functools.lru_cache(maxsize=None)
def planted(seed=0):
    """(rows (E,2) int64 shuffled, mag, ang (E,) float32, w (n,) float32, n): the row lengths of ROW_LENGTHS, rows 9..49 of 4 to 24
    slots, rows 50..69 empty; self rows [a, a] at the origin, neighbours of weight 0, duplicate rows"""
    rng = np.random.default_rng(seed)
    n = N_PLANTED
    rows, mag, ang = [], [], []

    def add(a, b, m, t):
        rows.append((a, b)), mag.append(m), ang.append(t)
    for a in range(50):
        count = ROW_LENGTHS.get(a, int(rng.integers(4, 25)))
        others = np.array([b for b in range(n) if b != a])
        for j in range(count):
            add(a, int(rng.choice(others)), rng.uniform(0.1, 1.0), rng.uniform(-np.pi, np.pi))
        if a == 2:          # two neighbours on one line through the origin
            ang[-2], ang[-1] = 0.3, 0.3 + np.pi
        if a == 3:
            ang[-2], ang[-1] = 0.3, 1.9
        if count >= 4:          # two of the counted slots are inactive: a neighbour of weight 0 and the row [a, a] at the origin
            rows[-1] = (a, ZERO_WEIGHT[a % 2])
            rows[-2], mag[-2], ang[-2] = (a, a), 0.0, 0.0
    base = len(rows)
    for j in rng.integers(0, base, 12):          # duplicate rows: one more term each
        if ROW_LENGTHS.get(rows[j][0]) is None:
            add(rows[j][0], rows[j][1], mag[j], ang[j])
    rows, mag, ang = np.array(rows, dtype=np.int64), np.array(mag, dtype=F32), np.array(ang, dtype=F32)
    shuffle = rng.permutation(len(rows))
    w = rng.uniform(0.5, 2.0, n).astype(F32)
    w[list(ZERO_WEIGHT)] = 0
    return rows[shuffle], mag[shuffle], ang[shuffle], w, n


def features(n, C, complex_x, seed):
    """float32-representable values"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C)).astype(F32)
    return (x + 1j * rng.standard_normal((n, C)).astype(F32)).astype(np.complex64) if complex_x else x


# ------------------------------------------------------------------ meshes with exact log maps
def planar_rows(pos, radius, theta=None):
    """every ordered pair (a, b), b != a, of a planar point set (z = 0) closer than radius, with the exact log vector of b at a in
    a's frame: the x axis turned by theta[a] -> (rows, mag, ang) in float64"""
    xy = pos[:, :2].astype(np.float64)
    d = xy[None, :, :] - xy[:, None, :]
    dist = np.hypot(d[..., 0], d[..., 1])
    a, b = np.nonzero((dist < radius) & (dist > 0))
    ang = np.arctan2(d[a, b, 1], d[a, b, 0])
    if theta is not None:
        ang = ang - theta[a]
    return np.stack((a, b), 1).astype(np.int64), dist[a, b], ang


def sphere_frames(pos):
    """(normal, e1, e2) in float64 on the unit sphere: the package's rule with normal = pos"""
    nrm = pos.astype(np.float64)
    nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
    ref = np.where(np.abs(nrm[:, 2:3]) < 0.95, np.array([0.0, 0.0, 1.0]), np.array([1.0, 0.0, 0.0]))
    e1 = np.cross(ref, nrm)
    e1 = e1 / np.linalg.norm(e1, axis=1, keepdims=True)
    return nrm, e1, np.cross(nrm, e1)


def sphere_rows(pos, radius):
    """every ordered pair (a, b), b != a, of points of the unit sphere at geodesic distance below radius, with the closed-form log
    map of b at a in sphere_frames -> (rows, mag, ang) in float64"""
    nrm, e1, e2 = sphere_frames(pos)
    cosd = np.clip(nrm @ nrm.T, -1.0, 1.0)
    dist = np.arccos(cosd)
    a, b = np.nonzero((dist < radius) & ~np.eye(len(nrm), dtype=bool))
    t = nrm[b] - cosd[a, b][:, None] * nrm[a]          # the direction of b in a's tangent plane
    ang = np.arctan2((t * e2[a]).sum(1), (t * e1[a]).sum(1))
    return np.stack((a, b), 1).astype(np.int64), dist[a, b], ang


def mean_edge_length(pos, face):
    p = pos.astype(np.float64)
    sides = np.concatenate([np.linalg.norm(p[face[i]] - p[face[(i + 1) % 3]], axis=1) for i in range(3)])
    return float(sides.mean())


class Plan64(Plan):
    """a plan whose geometry is given in float64 (the host tests): no float32 inputs in between"""

    def __init__(self, rows, mag, ang, n, w=None, rcond=RCOND):
        self.n, self.w, self.rcond = n, w, rcond
        self.by_query, self.rowptr, self.col, self.by_nbr, self.rowptr_t, self.col_t = csr(rows, n)
        self.mag, self.ang = np.asarray(mag, dtype=np.float64)[self.by_query], np.asarray(ang, dtype=np.float64)[self.by_query]
