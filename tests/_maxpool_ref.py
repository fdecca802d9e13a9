"""numpy restatement of max pooling by magnitude (csrc/fc_maxpool.hip): the key, the (key, slot) order, the winners, values and
gradients of tangent_transfer_max over a plan's rows and of mesh_max over the meshes of a batch, in float32 (the kernels'
arithmetic) and in float64 (the yardstick), and the step that plants ties.  Plans and features come from _transfer_ref, imported
unchanged.  Uses nothing from the package."""
import numpy as np

import _transfer_ref as tref

COMPLEX = tref.COMPLEX
ORIGIN = 1e-7          # reference utils/field.py:8: both components strictly inside (-1e-7, 1e-7)


# ------------------------------------------------------------------ key and order
def key(x, real):
    """complex x: fl(fl(re * re) + fl(im * im)) in `real`, every operation rounded on its own (numpy does not fuse); real x: x"""
    if not np.iscomplexobj(x):
        return np.asarray(x, dtype=real)
    re, im = np.asarray(x.real, dtype=real), np.asarray(x.imag, dtype=real)
    a, b = re * re, im * im
    k = a + b
    assert k.dtype == np.dtype(real)
    return k


def beats(kn, sn, k, s):
    """does the candidate (kn, sn) replace the incumbent (k, s)?  s < 0: no incumbent.  Elementwise."""
    return (sn >= 0) & ((s < 0) | (kn > k) | ((kn == k) & (sn < s)))


def combine(cands):
    """the winner (k, s) of a sequence of candidates (k, s), taken in the order given, by the rule of beats()"""
    k, s = None, -1
    for kn, sn in cands:
        if beats(kn, sn, 0 if k is None else k, s):
            k, s = kn, sn
    return k, s


# ------------------------------------------------------------------ over the rows of a plan
def transfer_winners(rows, n_out, x, real):
    """arg (n_out, C) int64: the winning slot of the forward CSR (rows grouped by out, stable) per output row and channel, -1 for a
    row without slots; the keys are taken in `real`, the scalar type of the features"""
    r = rows[tref.grouped(rows)]
    k = key(x, real)
    C = x.shape[1]
    arg = np.full((n_out, C), -1, dtype=np.int64)
    best = np.zeros((n_out, C), dtype=real)
    for e, (o, i) in enumerate(r):
        take = beats(k[i], np.full(C, e), best[o], arg[o])
        best[o] = np.where(take, k[i], best[o])
        arg[o] = np.where(take, e, arg[o])
    return arg


def units(rows, phase, conj, real):
    """(E,) the unit complex number of every forward slot in the arithmetic of `real`: phase, conj(phase), or 1"""
    order = tref.grouped(rows)
    if phase is None:
        return np.ones(len(rows), dtype=COMPLEX[np.dtype(real)])
    u = phase[order].astype(COMPLEX[np.dtype(real)])
    return np.conj(u) if conj else u


def transfer_forward(rows, phase, conj, x, arg, real):
    """y (n_out, C) on the winners `arg`: u[e*] * x[in(e*)] in the arithmetic of `real` for complex x; x[in(e*)] itself for real x
    (x must then already be of the dtype under test); 0 where arg is -1"""
    r = rows[tref.grouped(rows)]
    have = arg >= 0
    e = np.where(have, arg, 0)
    cols = np.broadcast_to(np.arange(x.shape[1]), arg.shape)
    if not np.iscomplexobj(x):
        return np.where(have, x[r[e, 1], cols], np.zeros((), dtype=x.dtype))
    dt = COMPLEX[np.dtype(real)]
    y = units(rows, phase, conj, real)[e] * x.astype(dt)[r[e, 1], cols]
    assert y.dtype == dt
    return np.where(have, y, np.zeros((), dtype=dt))


def transfer_backward(rows, phase, conj, n_in, gy, arg, real):
    """gx (n_in, C): over the slots t of the transposed CSR (grouped by in, stable, from the forward slot order) in ascending order,
    conj(u) * gy[out] added to a zero where the slot is the winner of (out, channel); real gy: gy[out] alone"""
    r = rows[tref.grouped(rows)]
    complex_x = np.iscomplexobj(gy)
    dt = COMPLEX[np.dtype(real)] if complex_x else real
    g = gy.astype(dt)
    u = np.conj(units(rows, phase, conj, real)) if complex_x else None
    gx = np.zeros((n_in, gy.shape[1]), dtype=dt)
    for e in np.argsort(r[:, 1], kind='stable'):
        o, i = r[e]
        won = arg[o] == e
        if won.any():
            term = u[e] * g[o] if complex_x else g[o]
            gx[i] = np.where(won, gx[i] + term, gx[i])
    assert gx.dtype == dt
    return gx


def winner_rows(rows, arg):
    """(n_out, C) int64: the input row of every winner, -1 where there is none"""
    r = rows[tref.grouped(rows)]
    return np.where(arg >= 0, r[np.where(arg >= 0, arg, 0), 1], -1)


def top_ties(rows, n_out, x, real):
    """how many (output row, channel) pairs have their largest key in two or more slots"""
    r = rows[tref.grouped(rows)]
    k = key(x, real)
    arg = transfer_winners(rows, n_out, x, real)
    n = 0
    for o in range(n_out):
        mine = np.nonzero(r[:, 0] == o)[0]
        if len(mine) > 1:
            top = k[r[arg[o], 1], np.arange(x.shape[1])]
            n += int(((k[r[mine, 1]] == top).sum(0) > 1).sum())
    return n


def plant_ties(rows, n_out, x, seed=0, every=3):
    """a copy of x with ties at the top: in every `every`-th output row with two or more distinct members (none of them used by an
    earlier step), the member that wins channel 0 is copied over another member of that row -- as it is, negated, or times i in
    turn: exactly the same key, since floating-point addition commutes.  Real x: copied as it is; and one more output row gets
    -0.0 and +0.0 as its two largest entries of channel 0, -0.0 in the earlier slot."""
    rng = np.random.default_rng(seed)
    x = x.copy()
    r = rows[tref.grouped(rows)]
    complex_x = np.iscomplexobj(x)
    factors = (1, -1, 1j) if complex_x else (1,)
    touched, n, zero_done = set(), 0, complex_x          # touched: the entries earlier steps rely on
    for o in range(n_out):
        members = r[r[:, 0] == o, 1]
        free = [m for m in dict.fromkeys(members) if m not in touched]
        if len(free) < 2 or len(free) < len(set(members)):
            continue
        if not zero_done:
            x[members, 0] = -np.abs(x[members, 0]) - 1
            x[free[0], 0], x[free[1], 0] = -0.0, 0.0
            zero_done = True
            touched |= set(members)
            continue
        n += 1
        if n % every:
            continue
        w = members[int(np.argmax(key(x[members, :1], x.real.dtype)[:, 0]))]
        d = rng.choice([m for m in free if m != w])
        x[d] = x[w] * factors[(n // every) % len(factors)]
        touched |= {w, d}
    return x


# ------------------------------------------------------------------ over the meshes of a batch
def mesh_winners(x, ptr, real, chunk=None):
    """idx (B, C) int64: the winning row of every mesh and channel, -1 for an empty mesh.  chunk=None: a plain argmax (the first of
    equal keys).  chunk=n: partial winners of every n rows counted from the mesh's first row, then combined by beats()."""
    k = key(x, real)
    B, C = len(ptr) - 1, x.shape[1]
    idx = np.full((B, C), -1, dtype=np.int64)
    for b in range(B):
        p0, p1 = int(ptr[b]), int(ptr[b + 1])
        if p1 == p0:
            continue
        if chunk is None:
            idx[b] = p0 + np.argmax(k[p0:p1], axis=0)
            continue
        best = np.zeros(C, dtype=real)
        for q0 in range(p0, p1, chunk):
            q1 = min(q0 + chunk, p1)
            s = q0 + np.argmax(k[q0:q1], axis=0)
            kn = k[s, np.arange(C)]
            take = beats(kn, s, best, idx[b])
            best, idx[b] = np.where(take, kn, best), np.where(take, s, idx[b])
    return idx


def origin(z):
    return (np.abs(z.real) < ORIGIN) & (np.abs(z.imag) < ORIGIN)


def mesh_forward(x, idx, real):
    """out (B, C) real on the winners idx: softAbs(x[n*]) = sqrt(key) outside the origin box and 0 inside, in the arithmetic of
    `real`, for complex x; x[n*] itself for real x; 0 where idx is -1"""
    have = idx >= 0
    n = np.where(have, idx, 0)
    cols = np.broadcast_to(np.arange(x.shape[1]), idx.shape)
    if x.shape[0] == 0:
        return np.zeros(idx.shape, dtype=real if np.iscomplexobj(x) else x.dtype)
    z = x[n, cols]
    if not np.iscomplexobj(x):
        return np.where(have, z, np.zeros((), dtype=x.dtype))
    out = np.where(origin(z), np.zeros((), dtype=real), np.sqrt(key(z, real)))
    assert out.dtype == np.dtype(real)
    return np.where(have, out, np.zeros((), dtype=real))


def mesh_backward(x, idx, g, real):
    """gx (N, C): g[b,c] * x / |x| at the winner outside the origin box (complex x), g[b,c] at the winner (real x), 0 elsewhere"""
    complex_x = np.iscomplexobj(x)
    gre, gim = np.zeros(x.shape, dtype=real), np.zeros(x.shape, dtype=real)
    gr = g.astype(real)
    for b, c in zip(*np.nonzero(idx >= 0)):
        n = idx[b, c]
        if not complex_x:
            gre[n, c] = gr[b, c]
        elif not origin(x[n, c]):
            re, im = real(x[n, c].real), real(x[n, c].imag)
            q = gr[b, c] / np.sqrt(re * re + im * im)
            gre[n, c], gim[n, c] = re * q, im * q
    return (gre + 1j * gim).astype(COMPLEX[np.dtype(real)]) if complex_x else gre


MESH_ROWS = (0, 1, 63, 64, 65, 129, 4200)          # the last has 66 chunks of 64 rows: more than one wavefront of partial winners


def mesh_case(C, complex_x, seed=0, rows=MESH_ROWS):
    """(x (N, C) float32-representable, ptr (B+1,) int64) with ties at the top (a winner copied to a later and an earlier row of its
    mesh: as it is, negated, times i), entries inside the origin box in every mesh, and -- the mesh of 63 rows -- a mesh that lies
    inside the box altogether, so that its winner does.  Real x: repeated values, and -0.0 before +0.0 as the top of a channel."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate(([0], np.cumsum(rows))).astype(np.int64)
    x = tref.features(int(ptr[-1]), C, complex_x, seed + 100)
    x = x.astype(np.complex64 if complex_x else np.float32)
    for b, n in enumerate(rows):
        p0 = int(ptr[b])
        if n < 3:
            continue
        if complex_x:
            x[p0 + rng.integers(0, n, max(n // 8, 1))] *= np.float32(1e-8)          # inside the origin box
            if n == 63:
                x[p0:p0 + n] *= np.float32(1e-8)
        top = p0 + np.argmax(key(x[p0:p0 + n], np.float32), axis=0)               # per channel
        for c in range(C):
            t = int(top[c])
            others = [p for p in (p0 + (t - p0 + n // 2) % n, p0 + (t - p0 + n - 1) % n) if p != t]
            f = ((1, -1, 1j)[c % 3]) if complex_x else 1
            for p in others[:1 + c % 2]:
                x[p, c] = x[t, c] * f
    if not complex_x:
        p0 = int(ptr[3])          # the mesh of 64 rows, channel 0: every entry negative but -0.0 and, after it, +0.0
        x[p0:p0 + 64, 0] = -np.abs(x[p0:p0 + 64, 0]) - 1
        x[p0 + 5, 0], x[p0 + 40, 0] = -0.0, 0.0
    return x, ptr
