"""numpy restatement of fieldconv_amd.transfer (csrc/fc_transfer.hip): the sparse transfer in float32 (the kernel's order: a row's
terms added to a zero in slot order) and in float64 (the yardstick), sample_cells, and the rows and weights of level_transfer.
Built on _geodesic_ref (distances, tight-edge labels, fixed-order sums), _logmap_ref and _diagonal_graph_ref (the transport
phase), imported unchanged.  Uses nothing from the package."""
import numpy as np

import _diagonal_graph_ref as dref
import _geodesic_ref as gref
import _logmap_ref as lref

F32 = np.float32
COMPLEX = {np.dtype(np.float32): np.complex64, np.dtype(np.float64): np.complex128}


# ------------------------------------------------------------------ the operator
def grouped(rows):
    """the slot order: rows grouped by out with a stable sort"""
    return np.argsort(rows[:, 0], kind='stable')


def coefficients(weight, phase, conj, real, complex_x):
    """(E,) coefficients in the arithmetic of `real`: the weight and the phase are cast first, then multiplied"""
    w = weight.astype(real)
    if not complex_x:
        return w
    if phase is None:
        return w.astype(COMPLEX[np.dtype(real)])
    ph = phase.astype(COMPLEX[np.dtype(real)])
    return w * (np.conj(ph) if conj else ph)


def transfer(rows, weight, phase, conj, n_out, x, real):
    """y (n_out, C) = T x in the arithmetic of `real` (np.float32 or np.float64): every product and every addition rounded to
    it, a row's terms added to a zero in slot order"""
    complex_x = np.iscomplexobj(x)
    dt = COMPLEX[np.dtype(real)] if complex_x else real
    coef = coefficients(weight, phase, conj, real, complex_x)
    xs = x.astype(dt)
    y = np.zeros((n_out, x.shape[1]), dtype=dt)
    for e in grouped(rows):
        o, i = rows[e]
        y[o] = y[o] + coef[e] * xs[i]
    assert y.dtype == dt
    return y


def adjoint(rows, weight, phase, conj, n_in, g, real):
    """T^H g in the kernel's order on the transposed CSR: grouped by in, a row's slots in the forward slot order"""
    order = grouped(rows)
    r = rows[order]
    ph = None if phase is None else phase[order]
    return transfer(r[:, ::-1], weight[order], ph, not conj, n_in, g, real)


def dense(rows, weight, phase, conj, n_out, n_in, complex_x=True):
    T = np.zeros((n_out, n_in), dtype=np.complex128 if complex_x else np.float64)
    coef = coefficients(weight, phase, conj, np.float64, complex_x)
    np.add.at(T, (rows[:, 0], rows[:, 1]), coef)
    return T


# ------------------------------------------------------------------ cells and the plans of a level pair
def graph_of(pos, face, diagonals=False):
    return dref.edge_graph(pos, face) if diagonals else gref.edge_graph(pos, face)


def sample_cells(pos, face, sample_idx, coarse, diagonals=False, graph=None):
    """(cell (S_f,) int64, dist (S_f,) float32): the tight-edge label of every fine sample's vertex among sample_idx[coarse]"""
    ptr, nbr, length = graph_of(pos, face, diagonals) if graph is None else graph
    sources = sample_idx[coarse]
    d = gref.dijkstra32(ptr, nbr, length, sources)
    label = gref.tight_labels(ptr, nbr, length, d, sources)
    return label[sample_idx], d[sample_idx]


def pool_weights(cell, w_fine, S_c):
    """(member, c, weight float32): w_fine[f] / W_c with W_c the float32 sum of the cell in ascending f; 1 / n_c where W_c == 0"""
    w = np.asarray(w_fine, dtype=F32).reshape(-1)
    total = gref.ordered_sums(w, cell, S_c)
    member = np.nonzero(cell >= 0)[0]
    c = cell[member]
    count = np.bincount(c, minlength=S_c).astype(F32)
    with np.errstate(divide='ignore', invalid='ignore'):
        weight = np.where(total[c] == 0, F32(1) / count[c], w[member] / total[c])
    assert weight.dtype == F32
    return member, c, weight


class Level:
    """the restated level pair: cells, rows, weights and -- per dtype -- the transport phases"""

    def __init__(self, pos, face, sample_idx, coarse, w_fine, diagonals=False):
        self.S_f, self.S_c = len(sample_idx), len(coarse)
        self.cell, self.dist = sample_cells(pos, face, sample_idx, coarse, diagonals)
        self.member, self.c, self.weight = pool_weights(self.cell, w_fine, self.S_c)
        self.n_outside = self.S_f - len(self.member)
        self.pool_rows = np.stack((self.c, self.member), 1)
        self.unpool_rows = np.stack((self.member, self.c), 1)
        far = self.dist[self.member].max() if len(self.member) else F32(0)
        self.bound = float(np.nextafter(F32(far), F32(np.inf))) if far > 0 else None
        self.case = None
        if self.bound is not None:
            edges = np.stack((coarse[self.c], self.member), 1)
            cls = dref.GraphCase if diagonals else lref.Case
            self.case = cls(pos, face, sample_idx, edges, self.bound)

    def xp(self, real):
        """(E,) complex phases of the member rows in the arithmetic of `real`"""
        if self.case is None:
            return np.ones(len(self.member), dtype=COMPLEX[np.dtype(real)])
        X = self.case.values(real)[1]
        return (X[:, 0] + 1j * X[:, 1]).astype(COMPLEX[np.dtype(real)])

    def pool(self, x, real, phase_real=None):
        ph = self.xp(real if phase_real is None else phase_real)
        return transfer(self.pool_rows, self.weight, ph, True, self.S_c, x, real)

    def unpool(self, x, real, phase_real=None):
        ph = self.xp(real if phase_real is None else phase_real)
        return transfer(self.unpool_rows, np.ones(len(self.member), dtype=F32), ph, False, self.S_f, x, real)


# ------------------------------------------------------------------ shared cases
def random_plan(seed=0, n_out=40, n_in=300, E=900, long_row=7, long_slots=200):
    """rows given unsorted, with empty output rows, one output row of `long_slots` slots and duplicate rows"""
    rng = np.random.default_rng(seed)
    empty = {3, 11, n_out - 1}
    allowed = np.array([o for o in range(n_out) if o not in empty and o != long_row])
    out = np.concatenate((np.full(long_slots, long_row), rng.choice(allowed, E - long_slots - 20)))
    inn = rng.integers(0, n_in, len(out))
    rows = np.stack((out, inn), 1)
    rows = np.concatenate((rows, rows[rng.integers(long_slots, len(rows), 20)]))          # 20 duplicate rows, none in the long row
    rows = rows[rng.permutation(len(rows))].astype(np.int64)
    assert len(rows) == E
    weight = rng.standard_normal(E).astype(F32)
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, E)).astype(np.complex64)
    return rows, weight, phase, sorted(empty)


def one_slot_plan(seed=1, n_out=300, n_in=40):
    """exactly one slot per output row: the shape of an unpool plan"""
    rng = np.random.default_rng(seed)
    rows = np.stack((rng.permutation(n_out), rng.integers(0, n_in, n_out)), 1).astype(np.int64)
    weight = rng.standard_normal(n_out).astype(F32)
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, n_out)).astype(np.complex64)
    return rows, weight, phase


def features(n, C, complex_x, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, C))
    return x + 1j * rng.standard_normal((n, C)) if complex_x else x


def flat_grid(n=12, h=0.125):
    return gref.lattice(n, n, h)
