"""Intrinsic gradient, divergence and Laplacian of per-sample features (csrc/fc_diffops.hip): the fixed, parameter-free
differential operators between real features (positions, logits, descriptors) and tangent-vector features.

    (G f)[a, c] = sum over the rows [a, b] of  k_ab * (f[b, c] - f[a, c])

is the weighted least-squares fit of a linear function to f over a's ball, in a's own tangent plane: the standard meshless
gradient.  For a row [a, b] of supp_edges, logMag and logAng are the polar coordinates of log_a(b) in a's frame, so the fit needs no
transport and its result -- a complex number per channel -- lives in a's frame: re-gauging a's frame by theta multiplies (G f)[a] by
exp(-i theta), as it does every tangent feature.  The coefficients k depend on the geometry alone (csrc/fc_diffops.hip states them),
so G is a sparse matrix built once per mesh, a GradientPlan, and applied in a fixed order without atomics.

    tangent_gradient(f, plan)      real (n, C) -> complex (n, C):   G f
    tangent_divergence(v, plan)    complex (n, C) -> real (n, C):   -W^-1 G^T W v, the negative adjoint of G in the W inner products
    laplacian(f, plan)             real (n, C) -> real (n, C):      tangent_divergence(tangent_gradient(f))

with W = diag(plan.w), the integration weights (data.w), or 1.  G^T is the transpose of G as a REAL-linear map:
Re<G f, v> = <f, G^T v>.  So sum_a w_a Re(conj(G f)_a v_a) = -sum_a w_a f_a (div v)_a, the Laplacian is symmetric and negative
semidefinite in the W inner product, and all three give exactly 0 on a constant.

Features are (n, C) tensors on the plan's ROCm device; there is no CPU or eager path.  Bad arguments raise before anything is
launched.  The geometry never receives a gradient; f and v do, when they require one."""
import math

import torch

from . import _lib
from ._launch import by_value as _by_value, device_of as _device_of, on as _on, ptr as _ptr, stream as _stream, whole as _whole

_REAL = {torch.float32: 0, torch.float64: 1}          # fc_dtype
_COMPLEX = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_COMPLEX_OF = {torch.float32: torch.complex64, torch.float64: torch.complex128}
RCOND = 1e-4


class GradientPlan(object):
    """The sparse gradient G (n x n) of one mesh or one MeshBatch, on a ROCm device.  Built by gradient_plan.

    n, n_slots        samples, and rows of supp_edges
    rowptr, col, coef     the CSR by query sample: (n+1,) int32, (n_slots,) int32 the neighbour, (n_slots,) complex64 its
                          coefficient; slots are the caller's rows grouped by query with a stable sort
    rowptr_t, col_t, coef_t   the transposed CSR, grouped by neighbour with a second stable sort: col_t is the query of a slot
    diag              (n,) complex64: the sum of a row's coefficients
    valid             (n,) uint8: 0 where the fit is degenerate -- no, one or only collinear neighbours -- and the row of G is zero
    n_invalid         0-dim int64 DEVICE tensor, the number of such rows: reading it synchronises, building it does not
    w                 (n,) float32, the integration weights the fit and the divergence use, or None for 1
    rcond             the threshold the rows were validated with"""

    def __init__(self, n, n_slots, rowptr, col, coef, rowptr_t, col_t, coef_t, diag, valid, n_invalid, w, rcond, device):
        self.n, self.n_slots, self.rcond, self.device = n, n_slots, rcond, device
        self.rowptr, self.col, self.coef, self.rowptr_t, self.col_t, self.coef_t = rowptr, col, coef, rowptr_t, col_t, coef_t
        self.diag, self.valid, self.n_invalid, self.w = diag, valid, n_invalid, w
        self._cast = {}

    def operands(self, real):
        """(coef, coef_t, diag, scale_in, scale_out) in the scalar type `real` (torch.float32 / float64), cast once and kept:
        scale_in = w (None without weights) and scale_out = -1 / w, 0 where w == 0 (-1 without weights), the two row scalings
        that make one adjoint launch the divergence."""
        if real not in self._cast:
            cplx = _COMPLEX_OF[real]
            with _on(self.device):
                if self.w is None:
                    s_in, s_out = None, torch.full((self.n,), -1.0, dtype=real, device=self.device)
                else:
                    s_in = self.w.to(real).contiguous()
                    s_out = torch.where(s_in == 0, torch.zeros_like(s_in), -1.0 / s_in).contiguous()
                self._cast[real] = (self.coef.to(cplx).contiguous(), self.coef_t.to(cplx).contiguous(), self.diag.to(cplx).contiguous(),
                                    s_in, s_out)
        return self._cast[real]

    def to(self, device):
        """The plan on another ROCm device (itself when it is there already)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'GradientPlan.to: a plan lives on a ROCm device, got {device}')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device == self.device:
            return self
        mv = lambda t: None if t is None else t.to(device)
        return GradientPlan(self.n, self.n_slots, mv(self.rowptr), mv(self.col), mv(self.coef), mv(self.rowptr_t), mv(self.col_t),
                            mv(self.coef_t), mv(self.diag), mv(self.valid), mv(self.n_invalid), mv(self.w), self.rcond, device)

    def __repr__(self):
        return 'GradientPlan(n={}, rows={}, rcond={}{})'.format(self.n, self.n_slots, self.rcond, '' if self.w is None else ', weighted')


def _check_rcond(rcond, what):
    try:
        ok = not isinstance(rcond, bool) and math.isfinite(float(rcond)) and 0 <= float(rcond) <= 1
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: rcond must be a number in [0, 1], got {rcond!r}')
    return float(rcond)


def gradient_plan(supp_edges, logMag, logAng, n, w=None, rcond=RCOND):
    """The GradientPlan of n samples from the rows [a, b] of supp_edges ((E,2) int64 positions in [0, n), in any order) with
    logMag, logAng ((E,) float32) the polar coordinates of log_a(b) in a's frame -- what ComputeLogXPort leaves on data -- and the
    integration weights w ((n,) or (n,1) float32, data.w; None for 1).

    Rows are grouped by query a with a stable sort: within a row the caller's order is kept, and a duplicate row is one more
    term of the fit.  A row [a, a], a neighbour of weight 0 and a row with a non-finite entry are inactive: coefficient 0.
    A query is valid iff det(A) > rcond * tr(A)^2 for the 2 x 2 moment matrix A of its ball (det / tr^2 <= 1/4 bounds the ratio
    of A's eigenvalues); an invalid query has a zero row in G.  plan.n_invalid counts them on the device.
    A MeshBatch is a union graph: the plan of the batch's fields is the plans of its meshes side by side.
    One launch (fc_gradient_coefficients), no atomics: two calls give the same bits.  The plan lives on logMag's device when that
    is a ROCm device, else on the current one."""
    what = 'gradient_plan'
    if not torch.is_tensor(supp_edges) or supp_edges.dim() != 2 or supp_edges.shape[1] != 2 or supp_edges.dtype != torch.int64:
        raise ValueError(f'{what}: supp_edges must be an (E,2) int64 tensor, got '
                         f'{(tuple(supp_edges.shape), supp_edges.dtype) if torch.is_tensor(supp_edges) else type(supp_edges).__name__}')
    E = int(supp_edges.shape[0])
    for t, name in ((logMag, 'logMag'), (logAng, 'logAng')):
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (E,):
            raise ValueError(f'{what}: {name} must be an ({E},) float32 tensor, one entry per row of supp_edges, got '
                             f'{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}')
    n = _whole(n, 0, 2 ** 31 - 2, what, 'n', integral_floats=True)
    if E >= 2 ** 31 - 1:
        raise ValueError(f'{what}: slots are 32-bit indices in the kernel: at most 2^31 - 2 rows, got {E}')
    if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) not in ((n,), (n, 1))):
        raise ValueError(f'{what}: w must be an ({n},) or ({n},1) float32 tensor or None, got '
                         f'{(tuple(w.shape), w.dtype) if torch.is_tensor(w) else type(w).__name__}')
    rcond = _check_rcond(rcond, what)
    if E and (int(supp_edges.min()) < 0 or int(supp_edges.max()) >= n):
        raise ValueError(f'{what}: supp_edges must hold positions in [0, {n})')
    dev = _device_of(logMag, 'gradient plans')
    lib = _lib.load()
    with _on(dev):
        r = supp_edges.detach().to(dev)
        order = torch.sort(r[:, 0], stable=True)
        query, by_query = order.values.contiguous(), order.indices
        nbr = r[by_query, 1].contiguous()
        mag, ang = logMag.detach().to(dev)[by_query].contiguous(), logAng.detach().to(dev)[by_query].contiguous()
        order = torch.sort(nbr, stable=True)          # the transposed matrix: grouped by neighbour, a row's slots in the order above
        nbr_sorted, by_nbr = order.values.contiguous(), order.indices
        ends = torch.arange(n + 1, device=dev)
        rowptr = torch.searchsorted(query, ends).to(torch.int32)
        rowptr_t = torch.searchsorted(nbr_sorted, ends).to(torch.int32)
        col, col_t = nbr.to(torch.int32), query[by_nbr].to(torch.int32).contiguous()
        wd = None if w is None else w.detach().to(dev).reshape(-1).contiguous()
        coef = torch.empty(E, dtype=torch.complex64, device=dev)
        diag = torch.empty(n, dtype=torch.complex64, device=dev)
        valid = torch.empty(n, dtype=torch.uint8, device=dev)
        _lib.check(lib.fc_gradient_coefficients(_ptr(rowptr), _ptr(col), _ptr(mag), _ptr(ang), _ptr(wd), rcond, n, E, _ptr(coef), _ptr(diag),
                                                _ptr(valid), _stream()), 'fc_gradient_coefficients')
        n_invalid = (valid == 0).sum()
        return GradientPlan(n, E, rowptr, col, coef, rowptr_t, col_t, coef[by_nbr].contiguous(), diag, valid, n_invalid, wd, rcond, dev)


def _apply(x, plan, coef):
    """G x of a checked, contiguous real device tensor"""
    C = int(x.shape[1])
    with _on(x.device):
        y = torch.empty((plan.n, C), dtype=_COMPLEX_OF[x.dtype], device=x.device)
        _lib.check(_lib.load().fc_gradient_apply(_ptr(x), _ptr(plan.rowptr), _ptr(plan.col), _ptr(coef), plan.n, plan.n_slots, C,
                                                 _REAL[x.dtype], _ptr(y), _stream()), 'fc_gradient_apply')
    return y


def _adjoint(g, plan, coef_t, diag, scale_in, scale_out):
    """scale_out * G^T (scale_in * g) of a checked, contiguous complex device tensor"""
    C = int(g.shape[1])
    real = _COMPLEX[g.dtype]
    with _on(g.device):
        gx = torch.empty((plan.n, C), dtype=real, device=g.device)
        _lib.check(_lib.load().fc_gradient_adjoint(_ptr(g), _ptr(plan.rowptr_t), _ptr(plan.col_t), _ptr(coef_t), _ptr(diag), _ptr(scale_in),
                                                   _ptr(scale_out), plan.n, plan.n_slots, C, _REAL[real], _ptr(gx), _stream()),
                   'fc_gradient_adjoint')
    return gx


class _TangentGradient(torch.autograd.Function):
    @staticmethod
    def forward(ctx, f, plan):
        ctx.plan = plan
        f = _by_value(f.detach())
        return _apply(f, plan, plan.operands(f.dtype)[0])

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        g = _by_value(g.detach())
        _, coef_t, diag, _, _ = ctx.plan.operands(_COMPLEX[g.dtype])
        return _adjoint(g, ctx.plan, coef_t, diag, None, None), None          # d/df of Re<g, G f> is G^T g


class _TangentDivergence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, v, plan):
        ctx.plan = plan
        v = _by_value(v.detach())
        _, coef_t, diag, s_in, s_out = plan.operands(_COMPLEX[v.dtype])
        return _adjoint(v, plan, coef_t, diag, s_in, s_out)

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        g = _by_value(g.detach())
        coef, _, _, s_in, s_out = ctx.plan.operands(g.dtype)
        with _on(g.device):          # d/dv of <g, S_out G^T S_in v> is S_in G (S_out g): the same two row scalings, applied here
            gv = _apply(g * s_out[:, None], ctx.plan, coef)
            return (gv if s_in is None else gv * s_in[:, None]), None


def _check(x, plan, what, name, complex_x):
    if not isinstance(plan, GradientPlan):
        raise ValueError(f'{what}: plan must be a GradientPlan, got {type(plan).__name__}')
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{what}: {name} must be an (n, C) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    if x.dtype not in (_COMPLEX if complex_x else _REAL):
        raise TypeError(f'{what}: {name} is {x.dtype}; ' + ('complex64 and complex128 (tangent features)' if complex_x else
                                                           'float32 and float64 (real features)') + ' are implemented')
    if not x.is_cuda:
        raise RuntimeError(f'{what}: {name} is on {x.device}; the operator runs on a ROCm device and has no CPU path')
    if x.device != plan.device:
        raise RuntimeError(f'{what}: {name} is on {x.device}, the plan on {plan.device}')
    if int(x.shape[0]) != plan.n or int(x.shape[1]) < 1:
        raise ValueError(f'{what}: {name} must be ({plan.n}, C) with C >= 1 for this plan, got {tuple(x.shape)}')
    if plan.n * int(x.shape[1]) >= 2 ** 40 or int(x.shape[1]) >= 2 ** 31:
        raise ValueError(f'{what}: n * C must stay below 2^40, got {plan.n} x {int(x.shape[1])}')


def tangent_gradient(f, plan):
    """G f (n, C) complex64 / complex128 for f (n, C) float32 / float64 on the plan's device: channel c of row a is the intrinsic
    gradient of f[:, c] at sample a as a complex number in a's frame.  y[a, c] = sum_e coef[e] * (f[col[e], c] - f[a, c]) over the
    slots of row a, added to a zero in slot order: one launch, no atomics, the same bits on every run; exactly 0 for a constant f,
    and for an invalid or empty row.  Applied to pos[sample_idx] it gives three tangent channels without a learned lift.
    Gradient flows to f only, and only when f requires one (one launch of the adjoint kernel on the transposed CSR, as
    deterministic as the forward pass).  A non-contiguous f is made contiguous.  A complex f raises TypeError."""
    _check(f, plan, 'tangent_gradient', 'f', False)
    return _TangentGradient.apply(f, plan)


def tangent_divergence(v, plan):
    """div v = -W^-1 G^T W v (n, C) float32 / float64 for v (n, C) complex64 / complex128 on the plan's device, W = plan.w or 1:
    the negative adjoint of tangent_gradient in the W inner products, sum_a w_a Re(conj(G f)_a v_a) = -sum_a w_a f_a (div v)_a up to
    rounding (plan.diag is the float32 sum of a row's coefficients: about 1e-8 of the inner product, in double too).  One launch of fc_gradient_adjoint with scale_in = w and scale_out = -1 / w (0 where w == 0): per row i the terms of
    the transposed CSR added to a zero in slot order, then the diagonal term subtracted.  No atomics, the same bits on every run.
    It does not depend on the samples' frames: re-gauging v with its frame leaves div v unchanged.  Gradient flows to v only, and
    only when v requires one.  A real v raises TypeError."""
    _check(v, plan, 'tangent_divergence', 'v', True)
    return _TangentDivergence.apply(v, plan)


def laplacian(f, plan):
    """tangent_divergence(tangent_gradient(f, plan), plan) for f (n, C) float32 / float64: a Laplacian of the sample graph that is
    symmetric and negative semidefinite in the W inner product -- sum_a w_a f_a (L f)_a = -sum_a w_a |G f|_a^2, the Dirichlet
    energy -- independent of the frames, and exactly 0 on constants.  Two launches forward, two backward."""
    return tangent_divergence(tangent_gradient(f, plan), plan)
