"""numpy restatement of fieldconv_amd.diffusion (csrc/fc_diffusion.hip): the active mask, the heat-kernel weights, the merged CSR of
the stiffness matrix S, S as a dense matrix, its application, the preconditioned CG recurrence for any dtype (vectors in the
dtype, every operation rounded on its own, the two inner products in float64 in the kernel's order), the adjoint solve and the
gradient of the diffusion times.  Every function takes `real`: np.float32 restates the kernels' arithmetic (only exp is numpy's,
not the device library's); np.float64 is the yardstick of both, computed from the same float32 inputs.  Also the planted case of
the device tests.  Uses nothing from the package."""
import functools

import numpy as np

F32 = np.float32
THREADS, LANES = 1024, 64
N_PLANTED = 67


# ------------------------------------------------------------------ the plan
def active_rows(rows, mag, xp, w):
    a, b = rows[:, 0], rows[:, 1]
    with np.errstate(invalid='ignore'):
        act = (a != b) & np.isfinite(mag) & (mag > 0) & np.isfinite(xp.real) & np.isfinite(xp.imag)
        if w is not None:
            ok = np.isfinite(w) & (w > 0)
            act = act & ok[a] & ok[b]
    return act


def default_h(mag, act):
    """fl32(the largest active logMag)^2 / 16, in double; 1 when no row is active"""
    top = float(mag[act].max()) if act.any() else 0.0
    return top * top / 16 if top > 0 else 1.0


def merged_csr(rows, n):
    """(rowptr, col, edge): row i holds its out entries (rows [i, b], ascending e), then its in entries (rows [a, i], ascending e);
    edge[k] = e for an in entry, -e - 1 for an out entry"""
    E = len(rows)
    rowptr, col, edge = np.zeros(n + 1, dtype=np.int32), [], []
    outs, ins = [[] for _ in range(n)], [[] for _ in range(n)]
    for e in range(E):
        outs[rows[e, 0]].append(e)
        ins[rows[e, 1]].append(e)
    for i in range(n):
        col += [rows[e, 1] for e in outs[i]] + [rows[e, 0] for e in ins[i]]
        edge += [-e - 1 for e in outs[i]] + list(ins[i])
        rowptr[i + 1] = len(col)
    return rowptr, np.array(col, dtype=np.int32).reshape(-1), np.array(edge, dtype=np.int32).reshape(-1)


def coefficients(rowptr, col, edge, rows, mag, xp, w, h, n, real):
    """(coef complex, coef_real, diag, diag_real) in the arithmetic of `real` from the float32 inputs"""
    act = active_rows(rows, mag, xp, w)
    four_h, norm = (real(F32(4.0 * h)), real(F32(4.0 * np.pi * h * h))) if real == F32 else (real(4.0 * h), real(4.0 * np.pi * h * h))
    K = len(col)
    cr, ci, g = np.zeros(K, dtype=real), np.zeros(K, dtype=real), np.zeros(K, dtype=real)
    diag, diag_real = np.zeros(n, dtype=real), np.zeros(n, dtype=real)
    half = real(0.5)
    for i in range(n):
        d, dr = real(0), real(0)
        for k in range(rowptr[i], rowptr[i + 1]):
            out = edge[k] < 0
            e = -(edge[k] + 1) if out else edge[k]
            if not act[e]:
                continue
            m, ur, ui = real(mag[e]), real(xp[e].real), real(xp[e].imag)
            wi, wj = (real(1), real(1)) if w is None else (real(w[i]), real(w[col[k]]))
            ce = ((wi * wj) * np.exp(-((m * m) / four_h))) / norm
            g[k] = -half * ce
            gi = g[k] * ui
            cr[k], ci[k] = g[k] * ur, (-gi if out else gi)
            d = d + (ce * (ur * ur + ui * ui) if out else ce)
            dr = dr + ce
        diag[i], diag_real[i] = half * d, half * dr
    assert cr.dtype == real and diag.dtype == real
    return cr + 1j * ci, g, diag, diag_real


class Plan(object):
    """the restated plan of (rows, xp, mag, n, w, h); values(real) -> (coef, coef_real, diag, diag_real)"""

    def __init__(self, rows, xp, mag, n, w=None, h=None):
        self.rows, self.xp, self.mag, self.n, self.w = rows, xp, mag, n, w
        self.active = active_rows(rows, mag, xp, w)
        self.h = default_h(mag, self.active) if h is None else float(h)
        self.rowptr, self.col, self.edge = merged_csr(rows, n)

    @functools.lru_cache(maxsize=None)
    def values(self, real):
        return coefficients(self.rowptr, self.col, self.edge, self.rows, self.mag, self.xp, self.w, self.h, self.n, real)

    def dense(self, complex_x=True, values=None):
        """S as a dense float64 / complex128 matrix from stored values (default: the float32 restatement's)"""
        coef, g, diag, diag_real = values if values is not None else self.values(F32)
        S = np.zeros((self.n, self.n), dtype=np.complex128 if complex_x else np.float64)
        for i in range(self.n):
            for k in range(self.rowptr[i], self.rowptr[i + 1]):
                S[i, self.col[k]] += np.complex128(coef[k]) if complex_x else np.float64(g[k])
            S[i, i] += np.float64(diag[i] if complex_x else diag_real[i])
        return S


# ------------------------------------------------------------------ vectors: (n, C, S) arrays of `real`, S = 2 (re, im) or 1
def split(x, real):
    return (np.stack([x.real, x.imag], -1) if np.iscomplexobj(x) else x[..., None]).astype(real)


def join(v):
    return v[..., 0] + 1j * v[..., 1] if v.shape[-1] == 2 else v[..., 0]


def entry_sum(rowptr, col, cr, ci, v, r0=0, nb=None):
    """acc[i] = sum over row i's entries of coef * v[col], added to a zero in entry order, every operation rounded on its own; an
    entry whose col lies outside [r0, r0 + nb) contributes nothing"""
    n = len(rowptr) - 1
    nb = n if nb is None else nb
    acc = np.zeros_like(v)
    length = rowptr[1:] - rowptr[:-1]
    for k in range(int(length.max()) if n else 0):
        i = np.nonzero(length > k)[0]
        e = rowptr[i] + k
        c = col[e]
        ok = (c >= r0) & (c < r0 + nb)
        i, e, c = i[ok], e[ok], c[ok]
        u = v[c]
        if v.shape[-1] == 2:
            a, b = cr[e, None] * u[..., 0], ci[e, None] * u[..., 1]
            cc, d = cr[e, None] * u[..., 1], ci[e, None] * u[..., 0]
            acc[i, :, 0] = acc[i, :, 0] + (a - b)
            acc[i, :, 1] = acc[i, :, 1] + (cc + d)
        else:
            acc[i, :, 0] = acc[i, :, 0] + cr[e, None] * u[..., 0]
    return acc


def operands(plan, complex_x, real, values=None):
    coef, g, diag, diag_real = values if values is not None else plan.values(F32)
    if complex_x:
        return coef.real.astype(real), coef.imag.astype(real), diag.astype(real)
    return g.astype(real), None, diag_real.astype(real)


def stiffness(plan, x, real, values=None, scale_in=None, scale_out=None):
    """scale_out * S (scale_in * x) as the apply kernel forms it"""
    cr, ci, d = operands(plan, np.iscomplexobj(x), real, values)
    v = split(x, real)
    if scale_in is not None:
        v = scale_in.astype(real)[:, None, None] * v
    out = entry_sum(plan.rowptr, plan.col, cr, ci, v) + d[:, None, None] * v
    if scale_out is not None:
        out = scale_out.astype(real)[:, None, None] * out
    assert out.dtype == real
    return join(out)


def laplacian_scale(plan, real):
    if plan.w is None:
        return np.full(plan.n, -1, dtype=real)
    w = plan.w.astype(real)
    with np.errstate(divide='ignore'):
        return np.where(w == 0, real(0), real(-1) / w)


def laplacian(plan, x, real, values=None):
    return stiffness(plan, x, real, values, None, laplacian_scale(plan, real))


def laplacian_adjoint(plan, g, real, values=None):
    return stiffness(plan, g, real, values, laplacian_scale(plan, real), None)


def block_dot(u, v):
    """Re<u, v> per channel in float64 in the kernel's order: thread l adds its rows l, l + 1024, ... (re then im) to a zero, the
    64 lanes of a wavefront are folded by halves, the 16 wavefronts are added in index order"""
    nb, C, S = u.shape
    pad = (-nb) % THREADS
    pr = u.astype(np.float64) * v.astype(np.float64)
    pr = np.concatenate([pr, np.zeros((pad, C, S))], 0).reshape(-1, THREADS, C, S)
    lane = np.zeros((THREADS, C))
    for j in range(pr.shape[0]):
        for s in range(S):
            lane = lane + pr[j, :, :, s]
    p = lane.reshape(THREADS // LANES, LANES, C)
    off = LANES // 2
    while off >= 1:
        p = p[:, :off] + p[:, off:2 * off]
        off //= 2
    total = np.zeros(C)
    for wv in range(THREADS // LANES):
        total = total + p[wv, 0]
    return total


def pcg(plan, x, t, real, iters, ptr=None, mode=0, values=None):
    """(out, lam, resid (B, C)): the kernel's recurrence per mesh.  mode 0: rhs = W x, y0 = x, out = y.  mode 1: rhs = x,
    y0 = x / w (0 where w <= 0), out = W y, lam = y."""
    complex_x = np.iscomplexobj(x)
    cr, ci, d = operands(plan, complex_x, real, values)
    n, C = x.shape
    ptr = [0, n] if ptr is None else [int(v) for v in ptr]
    w = np.ones(n, dtype=real) if plan.w is None else plan.w.astype(real)
    tc = t.astype(real)[None, :, None]
    xs = split(x, real)
    out, lam, resid = np.zeros_like(xs), np.zeros_like(xs), np.zeros((len(ptr) - 1, C), dtype=real)
    P = w[:, None, None] + tc * d[:, None, None]
    bad = ~((t >= 0) & np.isfinite(t))

    for b in range(len(ptr) - 1):
        r0, nb = ptr[b], ptr[b + 1] - ptr[b]
        rows = slice(r0, r0 + nb)
        full = np.zeros_like(xs)
        wb, db, Pb = w[rows, None, None], d[rows, None, None], P[rows]

        def A(v):
            full[rows] = v
            sx = entry_sum(plan.rowptr, plan.col, cr, ci, full, r0, nb)[rows] + db * v
            return wb * v + tc * sx

        def precondition(r):
            with np.errstate(divide='ignore', invalid='ignore'):
                return np.where(Pb > 0, r / Pb, real(0)).astype(real)
        if mode == 0:
            y, rhs = xs[rows].copy(), wb * xs[rows]
        else:
            with np.errstate(divide='ignore', invalid='ignore'):
                y, rhs = np.where(wb > 0, xs[rows] / wb, real(0)).astype(real), xs[rows].copy()
        r = rhs - A(y)
        z = precondition(r)
        p = z.copy()
        rz = block_dot(r, z)
        for _ in range(iters):
            q = A(p)
            pq = block_dot(p, q)
            with np.errstate(divide='ignore', invalid='ignore'):
                alpha = np.where(pq > 0, rz / pq, 0.0).astype(real)[None, :, None]
            y = np.where(alpha != 0, y + alpha * p, y)
            r = np.where(alpha != 0, r - alpha * q, r)
            z = precondition(r)
            rz_new = block_dot(r, z)
            with np.errstate(divide='ignore', invalid='ignore'):
                beta = np.where(rz > 0, rz_new / rz, 0.0).astype(real)[None, :, None]
            p = z + beta * p
            rz = rz_new
        assert y.dtype == real and p.dtype == real
        lam[rows] = y
        out[rows] = y if mode == 0 else wb * y
        with np.errstate(invalid='ignore'):
            resid[b] = np.sqrt(rz).astype(real)
    out[:, bad], lam[:, bad], resid[:, bad] = np.nan, np.nan, np.nan
    return join(out), join(lam), resid


def heat_diffuse(plan, x, t, real, iters, ptr=None, values=None):
    return pcg(plan, x, t, real, iters, ptr, 0, values)[0]


def heat_diffuse_backward(plan, x, t, gy, real, iters, ptr=None, values=None):
    """(gx, gt) by implicit differentiation: lambda = A^-1 gy by the same recurrence, gx = W lambda, gt = -Re <lambda, S y>"""
    y = heat_diffuse(plan, x, t, real, iters, ptr, values)
    gx, lam, _ = pcg(plan, gy, t, real, iters, ptr, 1, values)
    sy = stiffness(plan, y, real, values)
    gt = -np.sum((np.conj(lam).astype(np.complex128) * sy.astype(np.complex128)).real, 0)
    return gx, gt.astype(real)


def dense_solve(plan, x, t, values=None):
    """(W + t_c S)^-1 W x per channel in float64, one system of all n rows"""
    S = plan.dense(np.iscomplexobj(x), values)
    W = np.diag(np.ones(plan.n) if plan.w is None else plan.w.astype(np.float64))
    return np.stack([np.linalg.solve(W + float(t[c]) * S, W @ x[:, c].astype(S.dtype)) for c in range(x.shape[1])], 1)


# ------------------------------------------------------------------ the planted case of the device tests
@functools.lru_cache(maxsize=None)
def planted(seed=0):
    """(rows (E,2) int64, xp (E,) complex64, mag (E,) float32, w (n,) float32, n = 67): matrix rows of 0 (sample 0), 1 (sample 1: a
    one-directional row), 64 (sample 2), 65 (sample 3) and 130 (sample 4, with duplicates) entries, a self row (6), a zero-weight
    sample (7), inactive rows (zero and infinite length, a NaN transport), shuffled"""
    rng = np.random.RandomState(seed)
    n = N_PLANTED
    pairs, single = [], [(1, 5)]
    pairs += [(2, b) for b in range(10, 42)]                       # 32 pairs: 64 entries in row 2
    pairs += [(3, b) for b in range(20, 52)]                       # 32 pairs + one single row: 65 entries in row 3
    single += [(3, 60)]
    pairs += [(4, b) for b in range(10, 67)] + [(4, b) for b in range(10, 18)]          # 57 + 8 duplicates: 130 entries in row 4
    pairs += [(7, 8), (7, 9)]                                      # the zero-weight sample
    pairs += [(a, a + 1) for a in range(8, 66)] + [(a, a + 7) for a in range(8, 59, 3)]
    rows, xp = [], []
    for a, b in pairs:
        u = np.exp(1j * rng.uniform(-np.pi, np.pi))
        back = np.conj(u) if rng.rand() < 0.5 else np.exp(1j * rng.uniform(-np.pi, np.pi))
        rows += [(a, b), (b, a)]
        xp += [u, back]
    for a, b in single + [(6, 6)]:
        rows.append((a, b))
        xp.append(np.exp(1j * rng.uniform(-np.pi, np.pi)))
    rows, xp = np.array(rows, dtype=np.int64), np.array(xp).astype(np.complex64)
    mag = rng.uniform(0.05, 0.3, len(rows)).astype(F32)
    dead = [i for i in range(len(rows)) if rows[i, 0] >= 40 and rows[i, 1] >= 40][:3]
    mag[dead[0]], mag[dead[1]] = 0, np.inf
    xp[dead[2]] = np.nan
    order = rng.permutation(len(rows))
    rows, xp, mag = rows[order], xp[order], mag[order]
    w = rng.uniform(0.005, 0.02, n).astype(F32)
    w[7] = 0
    return rows, xp, mag, w, n


def features(n, C, complex_x, seed):
    rng = np.random.RandomState(seed)
    x = rng.standard_normal((n, C)) + (1j * rng.standard_normal((n, C)) if complex_x else 0)
    return x.astype(np.complex64 if complex_x else F32)


def times(C, scale=2e-3):
    """planted diffusion times: positive, one of them exactly 0 when C > 1"""
    t = (scale * (1 + np.arange(C) % 5)).astype(F32)
    if C > 1:
        t[1] = 0
    return t
