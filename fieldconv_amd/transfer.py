"""Tangent-feature pooling and unpooling between two sample levels (csrc/fc_transfer.hip): a sparse complex transfer

    y[o, c] = sum over the rows e with out(e) = o of  coef[e] * x[in(e), c]

with a deterministic gradient, the plan that holds its two CSRs, and the glue that builds the plans of a level pair from the
package's own geodesics: nearest-sample cells (geodesic.nearest_sample), sample masses (data.w) and the transport phase along a
shortest-path tree (logmap.log_map_transport).  interpolation_plan / vertex_interpolation build the smooth counterpart of the
unpool plan: every receiver from its k nearest coarse samples with inverse-distance weights (csrc/fc_interp.hip).
tangent_transfer_max is max pooling over the rows of a plan (csrc/fc_maxpool.hip): per output row and channel the ONE member of
largest magnitude, transported into the receiver's frame.

A tangent-vector feature lives in its sample's frame, so a plain mean over a cell is wrong: every term is parallel-transported
into the receiving sample's frame first, which is a multiplication by a unit complex number -- the phase of a row.  Real
(scalar) features, such as ECHOBlock descriptors and logits, are resampled with the weights alone.

Features are (N,C) tensors on a ROCm device; there is no CPU or eager path: a CPU feature tensor raises.  The geometry (plans,
cells) is built on the device whatever device its inputs are on.  Bad arguments raise ValueError before anything is launched.
weight and phase are geometry: they never receive a gradient."""
import torch

from . import _lib
from ._launch import by_value as _by_value, device_of as _device_of, on as _on, ptr as _ptr, stream as _stream, whole as _whole
from .geodesic import _batch_tables, _check_diagonals, _check_index, _check_mesh, _segment_sum, mesh_edge_graph, nearest_sample
from .logmap import _check_bound, log_map_transport

_DTYPES = {torch.float32: (0, 0), torch.float64: (1, 0), torch.complex64: (0, 1), torch.complex128: (1, 1)}          # (fc_dtype, is_complex)
_REAL = (torch.float32, torch.float64)
_COMPLEX = {torch.float32: torch.complex64, torch.float64: torch.complex128}


class _Csr(object):
    """One CSR by output row on the device: rowptr (n_rows+1,) int32, col (E,) int32, weight (E,) and phase (E,) or None in slot
    order; the casts of weight and phase to a feature's scalar type are made once and kept.  other (E,) int32: the slot number of
    every slot in the plan's other CSR (its transpose) -- what the gradient of a max needs to recognise a winning slot."""

    def __init__(self, rowptr, col, weight, phase, other=None):
        self.rowptr, self.col, self.weight, self.phase, self.other = rowptr, col, weight, phase, other
        self._cast = {}

    def coefficients(self, real):
        if real not in self._cast:
            self._cast[real] = (self.weight.to(real).contiguous(),
                                None if self.phase is None else self.phase.to(_COMPLEX[real]).contiguous())
        return self._cast[real]


class TransferPlan(object):
    """The sparse matrix T (n_out x n_in) of a transfer y = T x, T[out, in] = the sum of the coefficients of the rows [out, in].

    rows    (E,2) int64 [out, in], in any order; duplicates add
    weight  (E,) float32 or float64
    phase   (E,) complex64 or complex128, or None for 1
    conj_phase      the coefficient of a row is weight * conj(phase) in place of weight * phase (complex features; real
                    features always take the weight alone)

    Ranges, dtypes and lengths are checked (ValueError) before anything touches the device.  The rows are grouped by `out` with
    a stable sort -- a row's terms are added in the order the caller gave them -- and the transposed CSR, which the gradient
    runs on, is built from that order by a second stable sort: both once, both kept on the device (rows.device when that is a
    ROCm device, else the current one).  adjoint() is the plan of the conjugate-transposed matrix; it shares every buffer."""

    def __init__(self, rows, weight, phase=None, n_out=None, n_in=None, conj_phase=False):
        what = 'TransferPlan'
        if not torch.is_tensor(rows) or rows.dim() != 2 or rows.shape[1] != 2 or rows.dtype != torch.int64:
            raise ValueError(f'{what}: rows must be an (E,2) int64 tensor, got '
                             f'{(tuple(rows.shape), rows.dtype) if torch.is_tensor(rows) else type(rows).__name__}')
        E = int(rows.shape[0])
        if not torch.is_tensor(weight) or weight.dtype not in _REAL:
            raise ValueError(f'{what}: weight must be a float32 or float64 tensor, got '
                             f'{weight.dtype if torch.is_tensor(weight) else type(weight).__name__}')
        if tuple(weight.shape) != (E,):
            raise ValueError(f'{what}: weight must have one entry per row, ({E},), got {tuple(weight.shape)}')
        if phase is not None:
            if not torch.is_tensor(phase) or phase.dtype not in (torch.complex64, torch.complex128):
                raise ValueError(f'{what}: phase must be a complex64 or complex128 tensor or None, got '
                                 f'{phase.dtype if torch.is_tensor(phase) else type(phase).__name__}')
            if tuple(phase.shape) != (E,):
                raise ValueError(f'{what}: phase must have one entry per row, ({E},), got {tuple(phase.shape)}')
        if n_out is None or n_in is None:
            raise ValueError(f'{what}: n_out and n_in, the numbers of output and input rows, must be given')
        n_out = _whole(n_out, 0, 2 ** 31 - 2, what, 'n_out', integral_floats=True)
        n_in = _whole(n_in, 0, 2 ** 31 - 2, what, 'n_in', integral_floats=True)
        if E >= 2 ** 31 - 1:
            raise ValueError(f'{what}: slots are 32-bit indices in the kernel: at most 2^31 - 2 rows, got {E}')
        if not isinstance(conj_phase, bool):
            raise ValueError(f'{what}: conj_phase must be True or False, got {conj_phase!r}')
        if E:
            lo, hi = rows.min(0).values.tolist(), rows.max(0).values.tolist()
            if lo[0] < 0 or hi[0] >= n_out:
                raise ValueError(f'{what}: rows[:, 0] must lie in [0, {n_out}), got values from {lo[0]} to {hi[0]}')
            if lo[1] < 0 or hi[1] >= n_in:
                raise ValueError(f'{what}: rows[:, 1] must lie in [0, {n_in}), got values from {lo[1]} to {hi[1]}')
        dev = _device_of(rows, 'geodesics')
        with _on(dev):
            r = rows.detach().to(dev)
            w = weight.detach().to(dev)
            ph = None if phase is None else phase.detach().to(dev).resolve_conj()
            order = torch.sort(r[:, 0], stable=True)
            out_sorted, by_out = order.values.contiguous(), order.indices
            col = r[by_out, 1].contiguous()
            w, ph = w[by_out].contiguous(), None if ph is None else ph[by_out].contiguous()
            order = torch.sort(col, stable=True)          # the transposed matrix: grouped by `in`, a row's slots in the order above
            in_sorted, by_in = order.values.contiguous(), order.indices
            slots = torch.arange(E, dtype=torch.int32, device=dev)
            fwd = _Csr(torch.searchsorted(out_sorted, torch.arange(n_out + 1, device=dev)).to(torch.int32), col.to(torch.int32), w, ph,
                       torch.empty_like(slots).index_put_((by_in,), slots))          # transposed slot t holds forward slot by_in[t]
            bwd = _Csr(torch.searchsorted(in_sorted, torch.arange(n_in + 1, device=dev)).to(torch.int32),
                       out_sorted[by_in].to(torch.int32).contiguous(), w[by_in].contiguous(), None if ph is None else ph[by_in].contiguous(),
                       by_in.to(torch.int32).contiguous())
        self._set(fwd, bwd, n_out, n_in, E, conj_phase, dev)

    def _set(self, fwd, bwd, n_out, n_in, n_rows, conj_phase, device):
        self._fwd, self._bwd, self.n_out, self.n_in, self.n_rows, self.conj_phase, self.device = fwd, bwd, n_out, n_in, n_rows, conj_phase, device
        return self

    def adjoint(self):
        """The plan of T^H (n_in x n_out): the two CSRs swapped and the conjugate flag flipped; no copy."""
        return TransferPlan.__new__(TransferPlan)._set(self._bwd, self._fwd, self.n_in, self.n_out, self.n_rows, not self.conj_phase,
                                                        self.device)

    def rows(self):
        """(rows (E,2) int64 [out, in], weight (E,), phase (E,) or None) in slot order: grouped by out, the caller's order within
        a group; phase as given (conj_phase is not applied)."""
        c = self._fwd
        counts = (c.rowptr[1:] - c.rowptr[:-1]).to(torch.int64)
        out = torch.repeat_interleave(torch.arange(self.n_out, device=self.device), counts)
        return torch.stack((out, c.col.to(torch.int64)), 1), c.weight, c.phase

    def __repr__(self):
        return 'TransferPlan(n_out={}, n_in={}, rows={}{})'.format(self.n_out, self.n_in, self.n_rows, ', conj_phase=True' if self.conj_phase else '')


def _launch(x, plan):
    """y = T x of a checked, contiguous device tensor"""
    lib = _lib.load()
    dt, cplx = _DTYPES[x.dtype]
    C = int(x.shape[1])
    csr = plan._fwd
    w, ph = csr.coefficients(_REAL[dt])
    with _on(x.device):
        y = torch.empty((plan.n_out, C), dtype=x.dtype, device=x.device)
        _lib.check(lib.fc_transfer(_ptr(x), _ptr(csr.rowptr), _ptr(csr.col), _ptr(w), _ptr(ph) if cplx else None, int(plan.conj_phase and cplx),
                                   plan.n_out, plan.n_in, plan.n_rows, C, dt, cplx, _ptr(y), _stream()), 'fc_transfer')
    return y


class _TangentTransfer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        return _launch(_by_value(x.detach()), plan)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        plan = ctx.plan
        g = _by_value(g.detach())
        return _launch(g, plan.adjoint()), None          # d/dx of Re<gy, T x> is T^H gy: the same kernel on the transposed CSR


def _check_features(x, plan, what):
    """the checks of (x, plan) that every operator on a plan makes before it launches"""
    if not isinstance(plan, TransferPlan):
        raise ValueError(f'{what}: plan must be a TransferPlan, got {type(plan).__name__}')
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{what}: x must be an (n_in, C) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    if x.dtype not in _DTYPES:
        raise TypeError(f'{what}: x is {x.dtype}; complex64, float32, complex128 and float64 are implemented')
    if not x.is_cuda:
        raise RuntimeError(f'{what}: x is on {x.device}; the transfer runs on a ROCm device and has no CPU path')
    if x.device != plan.device:
        raise RuntimeError(f'{what}: x is on {x.device}, the plan on {plan.device}')
    if int(x.shape[0]) != plan.n_in or int(x.shape[1]) < 1:
        raise ValueError(f'{what}: x must be ({plan.n_in}, C) with C >= 1 for this plan, got {tuple(x.shape)}')
    if plan.n_out * int(x.shape[1]) >= 2 ** 40 or int(x.shape[1]) >= 2 ** 31:
        raise ValueError(f'{what}: n_out * C must stay below 2^40, got {plan.n_out} x {int(x.shape[1])}')


def tangent_transfer(x, plan):
    """y (n_out, C) = T x for x (n_in, C) complex64 / complex128 (coefficient weight * phase, or weight * conj(phase) for a plan
    with conj_phase) or float32 / float64 (coefficient weight), on the plan's ROCm device.  One launch, no atomics: a row's terms
    are added in the plan's slot order, two runs give the same bits, a row without terms is exactly zero.  Gradient flows to x
    only (the same kernel on plan.adjoint(), as deterministic as the forward pass), and only when x requires one.  A
    non-contiguous x is made contiguous."""
    _check_features(x, plan, 'tangent_transfer')
    return _TangentTransfer.apply(x, plan)


class _TangentTransferMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        lib = _lib.load()
        x = _by_value(x.detach())
        dt, cplx = _DTYPES[x.dtype]
        C = int(x.shape[1])
        csr = plan._fwd
        ph = csr.coefficients(_REAL[dt])[1] if cplx else None
        with _on(x.device):
            y = torch.empty((plan.n_out, C), dtype=x.dtype, device=x.device)
            arg = torch.empty((plan.n_out, C), dtype=torch.int32, device=x.device)
            _lib.check(lib.fc_transfer_max(_ptr(x), _ptr(csr.rowptr), _ptr(csr.col), _ptr(ph), int(plan.conj_phase and cplx), plan.n_out,
                                           plan.n_in, plan.n_rows, C, dt, cplx, _ptr(y), _ptr(arg), _stream()), 'fc_transfer_max')
        ctx.plan = plan
        ctx.save_for_backward(arg)
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, g, _):
        if not ctx.needs_input_grad[0]:
            return None, None
        lib = _lib.load()
        plan = ctx.plan
        arg, = ctx.saved_tensors
        g = _by_value(g.detach())
        dt, cplx = _DTYPES[g.dtype]
        C = int(g.shape[1])
        csr = plan._bwd
        ph = csr.coefficients(_REAL[dt])[1] if cplx else None
        with _on(g.device):
            gx = torch.empty((plan.n_in, C), dtype=g.dtype, device=g.device)
            _lib.check(lib.fc_transfer_max_backward(_ptr(g), _ptr(arg), _ptr(csr.rowptr), _ptr(csr.col), _ptr(csr.other), _ptr(ph),
                                                    int(plan.conj_phase and cplx), plan.n_out, plan.n_in, plan.n_rows, C, dt, cplx, _ptr(gx),
                                                    _stream()), 'fc_transfer_max_backward')
        return gx, None


def tangent_transfer_max(x, plan, return_indices=False):
    """y (n_out, C): max pooling by magnitude over the rows of a plan (csrc/fc_maxpool.hip), for x (n_in, C) complex64 / complex128 /
    float32 / float64 on the plan's ROCm device.  Output row o takes, per channel, ONE of the plan's rows [o, i]:

      key      of a complex entry: k = fl(fl(re * re) + fl(im * im)) in x's scalar type, every operation rounded on its own (numpy
               gives the same bits).  |x| does not depend on a sample's frame, so the choice is gauge invariant.  Of a real entry:
               k = x itself -- a plain max, not a magnitude max.
      winner   the slot e* of output row o (the plan's slot order: rows grouped by out, the caller's order within a group) with the
               largest key(x[in(e), c]); ties go to the smallest slot.  NaN features are outside the contract.
      value    complex x: y[o, c] = u[e*] * x[in(e*), c] with u the row's phase (conj(phase) for a plan with conj_phase, 1 without
               phases): the winner parallel-transported into the receiver's frame.  Real x: x[in(e*), c], copied bit for bit.

    The plan's weights are NOT read: a max is not weighted, every row of the plan is a member.  A row of y without terms is
    exactly zero.  With return_indices also (n_out, C) int64: the INPUT row in(e*) of every winner, -1 where there is none.
    One launch forward and one backward, no atomics, the same bits on every run.  Gradient flows to x only, and only when x
    requires one: gx[i, c] = the sum, over the outputs o that input i won, of conj(u) * gy[o, c] (real: gy[o, c]) in the transposed
    plan's slot order; an input that won nowhere gets exactly zero.  A non-contiguous x is made contiguous.  Arguments are checked
    as tangent_transfer checks them, before anything is launched."""
    what = 'tangent_transfer_max'
    _check_features(x, plan, what)
    if not isinstance(return_indices, bool):
        raise ValueError(f'{what}: return_indices must be True or False, got {return_indices!r}')
    y, arg = _TangentTransferMax.apply(x, plan)
    if not return_indices:
        return y
    with _on(x.device):
        slot = arg.to(torch.int64)
        if plan.n_rows == 0:
            return y, slot
        return y, torch.where(slot >= 0, plan._fwd.col.to(torch.int64)[slot.clamp(min=0)], slot)


# ------------------------------------------------------------------ building a level pair
def _check_coarse(coarse, S, what):
    """(S_c,) int64 strictly ascending positions in [0,S) -> its entries as Python ints"""
    _check_index(coarse, S, what, 'coarse')
    host = coarse.tolist()
    if any(b <= a for a, b in zip(host, host[1:])):
        raise ValueError(f'{what}: coarse must be strictly ascending positions in sample_idx')
    return host


def _check_batch(pos_ptr, ptr, coarse_ptr, V, S, host_c, what):
    """all three range tables or none -> (host pos_ptr, host ptr, host coarse_ptr) or (None, None, None)"""
    given = [t is not None for t in (pos_ptr, ptr, coarse_ptr)]
    if any(given) and not all(given):
        raise ValueError(f'{what}: pos_ptr, ptr and coarse_ptr go together (the ranges of a MeshBatch and of its coarse level): give all or none')
    if not any(given):
        return None, None, None
    _, _, hp, hs, _ = _batch_tables(pos_ptr, ptr, V, S, what, 'ptr')
    hc = _batch_tables(pos_ptr, coarse_ptr, V, len(host_c), what, 'coarse_ptr')[3]
    for b in range(len(hp) - 1):
        mine = host_c[hc[b]:hc[b + 1]]
        if not mine:
            raise ValueError(f'{what}: mesh {b} of the batch has no coarse samples')
        if mine[0] < hs[b] or mine[-1] >= hs[b + 1]:
            raise ValueError(f'{what}: the coarse samples of mesh {b} must be positions inside its own range [{hs[b]}, {hs[b + 1]}) of sample_idx')
    return hp, hs, hc


def sample_cells(pos, face, sample_idx, coarse, graph=None, diagonals=False, pos_ptr=None, ptr=None, coarse_ptr=None):
    """(cell (S_f,) int64, dist (S_f,) float32): which coarse sample every fine sample belongs to.  sample_idx (S_f,) int64
    are the fine samples (vertices of pos), coarse (S_c,) int64 strictly ascending POSITIONS in sample_idx.  cell[f] is the
    nearest_sample label of vertex sample_idx[f] among the vertices sample_idx[coarse] -- a position in coarse, -1 where no
    coarse sample is reachable -- and dist[f] its edge-graph distance (+inf there).  A pure composition of nearest_sample: its
    bits, its tie rule (the lower position), its graph= and diagonals=.  A coarse sample is in its own cell, at distance 0,
    unless a fine sample listed earlier names the same vertex.
    pos_ptr, ptr, coarse_ptr: all None, or the (B+1,) int64 range tables of a MeshBatch over pos, sample_idx and coarse: every
    mesh searches its own coarse samples only, so no cell crosses meshes."""
    what = 'sample_cells'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    host_c = _check_coarse(coarse, int(sample_idx.numel()), what)
    hp, hs, hc = _check_batch(pos_ptr, ptr, coarse_ptr, V, int(sample_idx.numel()), host_c, what)
    fine = sample_idx.to(pos.device)
    label, dist = nearest_sample(pos, face, fine[coarse.to(pos.device)], pos_ptr, coarse_ptr, graph=graph, diagonals=diagonals)
    return label[fine], dist[fine]


def level_transfer(pos, face, sample_idx, coarse, w_fine, graph=None, diagonals=False, pos_ptr=None, ptr=None, coarse_ptr=None, bound=None,
                   return_cells=False):
    """(pool_plan, unpool_plan) between the fine samples sample_idx (S_f,) and the coarse samples sample_idx[coarse] (S_c,);
    with return_cells also (cell, n_outside): sample_cells' labels and the number of fine samples in no cell.

    For a fine sample f with cell c >= 0 and a = coarse[c], the row [a, f] goes through log_map_transport(pos, face, sample_idx,
    rows, bound): its xp turns coordinates in a's frame into coordinates in f's frame after transport along the shortest-path
    tree of a.  bound defaults to the largest finite cell distance moved one float32 step upward, so that the strict threshold
    of the tree reaches every member of every cell; when that distance is 0 no tree is grown and every phase is 1.
      unpool  (S_f x S_c)  row [f, c], weight 1, phase xp: a coarse feature carried out to the members of its cell.
      pool    (S_c x S_f)  row [c, f], weight w_fine[f] / W_c with W_c the float32 sum of the cell's w_fine in ascending f (1 / n_c
                           for a cell of n_c members where W_c == 0), phase conj(xp): the mass-weighted mean of the cell in a's
                           frame.  The weights of a non-empty cell sum to 1, so pool(unpool(y)) = y.
    A fine sample with cell -1 belongs to no cell: pooling ignores it and unpooling gives it zero.
    w_fine: (S_f,) or (S_f,1) float32, the fine level's data.w.  graph, diagonals, pos_ptr / ptr / coarse_ptr: as in
    sample_cells (one graph is built and shared by both steps).  Plans live on the device; nothing here is differentiable."""
    what = 'level_transfer'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    S_f = int(sample_idx.numel())
    host_c = _check_coarse(coarse, S_f, what)
    S_c = len(host_c)
    _check_batch(pos_ptr, ptr, coarse_ptr, V, S_f, host_c, what)
    if not torch.is_tensor(w_fine) or w_fine.dtype != torch.float32 or tuple(w_fine.shape) not in ((S_f,), (S_f, 1)):
        raise ValueError(f'{what}: w_fine must be an ({S_f},) or ({S_f},1) float32 tensor, got '
                         f'{(tuple(w_fine.shape), w_fine.dtype) if torch.is_tensor(w_fine) else type(w_fine).__name__}')
    if bound is not None:
        bound = _check_bound(bound, what)
    dev = _device_of(pos, 'geodesics')
    if graph is None:
        graph = mesh_edge_graph(pos, face, diagonals)
    cell, dist = sample_cells(pos, face, sample_idx, coarse, graph=graph, pos_ptr=pos_ptr, ptr=ptr, coarse_ptr=coarse_ptr)
    with _on(dev):
        cell, dist = cell.to(dev), dist.to(dev)
        member = torch.nonzero(cell >= 0)[:, 0]          # ascending f
        c = cell[member]
        n_outside = S_f - int(member.numel())
        a = coarse.to(dev)[c]
        if bound is None:
            far = float(dist[member].max()) if member.numel() else 0.0
            bound = float(torch.nextafter(torch.tensor(far, dtype=torch.float32), torch.tensor(float('inf'), dtype=torch.float32))) if far > 0 else None
        if bound is None or not member.numel():
            xp = torch.ones(int(member.numel()), dtype=torch.complex64, device=dev)
        else:
            xp = log_map_transport(pos, face, sample_idx, torch.stack((a, member), 1), bound, graph=graph,
                                   pos_ptr=pos_ptr, ptr=ptr)[2].to(dev)
        w = w_fine.detach().to(dev).reshape(-1).contiguous()
        total = _segment_sum(w, cell, S_c, 1.0, dev)          # float32, ascending f; cell -1 contributes to nothing
        count = torch.bincount(c, minlength=S_c).to(torch.float32)
        weight = torch.where(total[c] == 0, 1.0 / count[c], w[member] / total[c])
        unpool = TransferPlan(torch.stack((member, c), 1), torch.ones_like(weight), xp, n_out=S_f, n_in=S_c)
        pool = TransferPlan(torch.stack((c, member), 1), weight, xp, n_out=S_c, n_in=S_f, conj_phase=True)
    return (pool, unpool, cell.to(pos.device), n_outside) if return_cells else (pool, unpool)


# ------------------------------------------------------------------ interpolation from the k nearest coarse samples
KNN_MAX = 16          # fc_knn_weights keeps a row's best k in registers: 1 <= k <= 16


def _check_knn(k, power, what):
    k = _whole(k, 1, KNN_MAX, what, 'k', integral_floats=True)
    if isinstance(power, bool) or power not in (1, 2):
        raise ValueError(f'{what}: power must be 1 or 2, got {power!r}')
    return k, int(power)


def knn_weights(rowptr, cand, dist, k=3, power=2):
    """(sel (n_f,k) int32, weight (n_f,k) float32) of csrc/fc_interp.hip (fc_knn_weights) for a CSR of candidates by receiving
    row: rowptr (n_f+1,) int32, cand (n_slots,) int32 coarse positions, dist (n_slots,) float32 >= 0 and finite, on a ROCm device.
    With m = min(k, row length), sel[f, :m] are the slots of the row's m smallest candidates by (dist, cand, slot), in that
    order, and weight[f, :m] their weights: 1, 0, ..., 0 when the nearest distance is 0, else u_i / s with q_i = d_i (power 1) or
    d_i * d_i (power 2), u_i = 1 / max(q_i, 1e-30) and s = ((u_0 + u_1) + u_2) + ..., every operation rounded to float32 on its
    own.  From rank m on sel is -1 and weight 0; an empty row has m = 0.  One launch, no atomics: two runs give the same bits."""
    what = 'knn_weights'
    k, power = _check_knn(k, power, what)
    for t, name, dt in ((rowptr, 'rowptr', torch.int32), (cand, 'cand', torch.int32), (dist, 'dist', torch.float32)):
        if not torch.is_tensor(t) or t.dim() != 1 or t.dtype != dt:
            raise ValueError(f'{what}: {name} must be a 1-D {dt} tensor, got {(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}')
    if rowptr.numel() < 1 or cand.shape != dist.shape:
        raise ValueError(f'{what}: rowptr must hold n_f + 1 entries and cand and dist one entry per slot, got {tuple(rowptr.shape)}, '
                         f'{tuple(cand.shape)} and {tuple(dist.shape)}')
    if not rowptr.is_cuda or cand.device != rowptr.device or dist.device != rowptr.device:
        raise RuntimeError(f'{what}: rowptr, cand and dist must be on one ROCm device; there is no CPU path')
    n_f, n_slots = int(rowptr.numel()) - 1, int(cand.numel())
    if n_f * k >= 2 ** 31:
        raise ValueError(f'{what}: n_f * k must stay below 2^31, got {n_f} x {k}')
    lib = _lib.load()
    rowptr, cand, dist = rowptr.contiguous(), cand.contiguous(), dist.contiguous()
    with _on(rowptr.device):
        sel = torch.empty((n_f, k), dtype=torch.int32, device=rowptr.device)
        weight = torch.empty((n_f, k), dtype=torch.float32, device=rowptr.device)
        _lib.check(lib.fc_knn_weights(_ptr(rowptr), _ptr(cand) if n_slots else None, _ptr(dist) if n_slots else None, n_f, n_slots, k, power,
                                      _ptr(sel), _ptr(weight), _stream()), 'fc_knn_weights')
    return sel, weight


def interpolation_plan(pos, face, sample_idx, coarse, k=3, power=2, radius=None, graph=None, diagonals=False, pos_ptr=None, ptr=None,
                       coarse_ptr=None, return_rows=False, *, _what='interpolation_plan'):
    """The TransferPlan (S_f x S_c) that carries features of the coarse samples sample_idx[coarse] (S_c,) to the fine samples
    sample_idx (S_f,) ascending as PointNet++'s feature propagation does: every fine sample receives the inverse-distance-weighted
    combination of its k nearest coarse samples, each term parallel-transported into the receiver's frame first.  Where
    level_transfer's unpool is piecewise constant over the cells, this is continuous across their boundaries.

    radius  None: fl32(2 far) moved one float32 step upward, far the largest finite sample_cells distance, so that a fine sample
            in a cell has at least its own coarse sample as a candidate.  When far == 0 every member is a coarse sample (or lies
            on one) and the plan is [f, cell[f]] with weight 1 and phase 1.  Given: a finite number > 0.
    candidates   every pair (c, f) with d_a[sample_idx[f]] < fl32(radius), strict, d_a the single-source field of vertex
            a = sample_idx[coarse[c]] bounded by radius: geodesic_radius_edges' relation, coarse queries only, never truncated.
            (Only the S_c coarse balls are solved: geodesic_radius_edges(..., queries=coarse).)
    rows    [coarse[c], f] go through log_map_transport(..., bound=radius): dist is its logMag, the distance the convolution
            sees, xp its phase.  Every row is reached by construction; that is checked.
    plan    per fine sample f its candidates ascending in c go to knn_weights(k, power); its m = min(k, candidates) rows [f, c_i]
            follow in rank order with weight w_i and phase xp_i (unpool's convention, conj_phase False).  The zero-weight rows of
            an exact hit are kept.  A fine sample without a candidate (cell -1, or further than radius from every coarse sample)
            has no row: zero output.
    graph, diagonals, pos_ptr / ptr / coarse_ptr: as in level_transfer; in a batch no candidate crosses meshes.
    return_rows: also (rowptr (S_f+1,) int32, cand (E,) int32, dist (E,) float32, xp (E,) complex64), the candidate CSR the
    selection ran on.  Nothing here is differentiable; the operator's gradient runs on plan.adjoint()."""
    what = _what
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    S_f = int(sample_idx.numel())
    if S_f > 1 and not bool((sample_idx[1:] > sample_idx[:-1]).all()):
        raise ValueError(f'{what}: sample_idx must be strictly ascending')
    host_c = _check_coarse(coarse, S_f, what)
    S_c = len(host_c)
    _check_batch(pos_ptr, ptr, coarse_ptr, V, S_f, host_c, what)
    k, power = _check_knn(k, power, what)
    if radius is not None:
        radius = _check_bound(radius, what)
    if not isinstance(return_rows, bool):
        raise ValueError(f'{what}: return_rows must be True or False, got {return_rows!r}')
    from .geodesic_sampling import geodesic_radius_edges
    dev = _device_of(pos, 'geodesics')
    if graph is None:
        graph = mesh_edge_graph(pos, face, diagonals)
    trivial = False
    if radius is None:
        cell, dist = sample_cells(pos, face, sample_idx, coarse, graph=graph, pos_ptr=pos_ptr, ptr=ptr, coarse_ptr=coarse_ptr)
        cell, dist = cell.to(dev), dist.to(dev)
        inside = (cell >= 0) & torch.isfinite(dist)
        far = float(dist[inside].max()) if bool(inside.any()) else 0.0
        if far > 0:
            up = torch.nextafter(torch.tensor(2.0, dtype=torch.float32) * torch.tensor(far, dtype=torch.float32),
                                 torch.tensor(float('inf'), dtype=torch.float32))
            radius = _check_bound(float(up), what)
        else:
            trivial = True
    with _on(dev):
        if trivial:          # no tree to grow: every member sits on its coarse sample
            f = torch.nonzero(inside)[:, 0]
            c = cell[f]
            mag = torch.zeros(int(f.numel()), dtype=torch.float32, device=dev)
            xp = torch.ones(int(f.numel()), dtype=torch.complex64, device=dev)
        else:
            edges = geodesic_radius_edges(pos, face, sample_idx, radius, max_num_neighbors=S_f, pos_ptr=pos_ptr, sample_ptr=ptr,
                                          graph=graph, queries=coarse).to(dev)          # S_f neighbours at most: the cap cannot bite
            a, f = edges[:, 0], edges[:, 1]
            c = torch.searchsorted(coarse.to(dev).contiguous(), a.contiguous())          # (coarse ascends: a's place in it)
            if int(f.numel()):
                mag, _, xp, reached = log_map_transport(pos, face, sample_idx, torch.stack((a, f), 1), radius, graph=graph, pos_ptr=pos_ptr,
                                                        ptr=ptr, return_reached=True)
                if not bool(reached.all()):
                    raise _lib.FieldConvNativeError(f'{what}: {int((~reached).sum())} candidate rows inside the radius were not reached by '
                                                    'the transport tree: the ball search and the log map disagree')
                mag, xp = mag.to(dev), xp.to(dev)
            else:
                mag = torch.zeros(0, dtype=torch.float32, device=dev)
                xp = torch.ones(0, dtype=torch.complex64, device=dev)
        order = torch.sort(f, stable=True)          # grouped by receiver; the rows came grouped by c ascending, so c ascends in a group
        rowptr = torch.searchsorted(order.values.contiguous(), torch.arange(S_f + 1, device=dev)).to(torch.int32)
        cand = c[order.indices].to(torch.int32).contiguous()
        mag, xp = mag[order.indices].contiguous(), xp[order.indices].contiguous()
        sel, w = knn_weights(rowptr, cand, mag, k, power)
        taken = sel >= 0
        slot = sel[taken].to(torch.int64)          # row-major: by receiver, then rank
        recv = torch.nonzero(taken)[:, 0]
        plan = TransferPlan(torch.stack((recv, cand[slot].to(torch.int64)), 1), w[taken], xp[slot], n_out=S_f, n_in=S_c)
    return (plan, rowptr, cand, mag, xp) if return_rows else plan


def vertex_interpolation(pos, face, sample_idx, k=3, power=2, radius=None, graph=None, diagonals=False, pos_ptr=None, ptr=None):
    """The TransferPlan (V x S) of interpolation_plan with every vertex of pos as the fine level and the samples sample_idx (S,)
    strictly ascending as the coarse one: it carries sample-level logits (real features take the weights alone) or tangent
    features, transported into vertex_frames, to the full mesh.  The row of a sampled vertex is the identity.  pos_ptr, ptr: both
    None, or the range tables of a MeshBatch over pos and sample_idx; no row crosses meshes."""
    what = 'vertex_interpolation'
    _check_mesh(pos, face, what)
    if (pos_ptr is None) != (ptr is None):
        raise ValueError(f'{what}: pos_ptr and ptr go together (the ranges of a MeshBatch): give both or neither')
    every = torch.arange(int(pos.shape[0]), dtype=torch.int64, device=sample_idx.device if torch.is_tensor(sample_idx) else None)
    return interpolation_plan(pos, face, every, sample_idx, k, power, radius, graph, diagonals, pos_ptr, pos_ptr, ptr, _what=what)
