"""Heat diffusion of per-sample features (csrc/fc_diffusion.hip): the connection Laplacian of a sample level and the learned
diffusion y = (I - t L)^-1 x of DiffusionNet, one diffusion time per channel, solved on the device by a fixed number of
preconditioned conjugate-gradient steps in ONE launch.

    S = 1/2 D^H C D,   (D v)[e] = v[b] - u_e v[a]   for a row e = [a, b] of supp_edges,   u_e = xp[e]
    c_e = w_a w_b exp(-m_e^2 / (4 h)) / (4 pi h^2),   m_e = logMag[e]          (the point-cloud heat kernel, float32)
    L = -W^-1 S,   W = diag(w)

u_e turns a's coordinates into b's after transport, so D compares a neighbour's value only after parallel transport: L is the
CONNECTION Laplacian, and everything built from it commutes with a change of the samples' frames.  Real features use the same
matrix with u = 1.  S is Hermitian positive semidefinite whatever the rows are (duplicates, one-directional rows), so

    heat_diffuse(x, t, plan)      y = (W + t S)^-1 W x     per mesh and channel, `iters` CG steps
    connection_laplacian(x, plan) L x

Features are (n, C) tensors on the plan's ROCm device; there is no CPU or eager path.  Bad arguments raise before anything is
launched.  The geometry never receives a gradient; x and t do, when they require one."""
import math

import torch

from . import _lib
from ._launch import by_value as _by_value, device_of as _device_of, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .pooling import check_ptr, ptr_on

_REAL = {torch.float32: 0, torch.float64: 1}          # fc_dtype
_COMPLEX = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_SCALAR = {torch.float32: torch.float32, torch.float64: torch.float64, **_COMPLEX}
# rows of a mesh whose search direction stays in LDS (fc_diffusion_lds_rows(): 16 bytes of a row per workgroup, whatever the dtype)
LDS_ROWS = {torch.float32: 10000, torch.float64: 10000, torch.complex64: 10000, torch.complex128: 10000}
MAX_ITERS = 1024


class DiffusionPlan(object):
    """The stiffness matrix S (n x n) of one mesh or one MeshBatch, on a ROCm device.  Built by diffusion_plan.

    n, n_entries      samples, and stored entries: two per row of supp_edges
    rowptr, col       the merged CSR: (n+1,) int32, (n_entries,) int32.  Row i holds its OUT entries (rows [i, b]: col b) in ascending
                      row order, then its IN entries (rows [a, i]: col a) in ascending row order
    edge              (n_entries,) int32: the row e of supp_edges an entry comes from; -e - 1 for an out entry
    coef, coef_real   (n_entries,) complex64 and float32: -1/2 c_e conj(u_e) (out) or -1/2 c_e u_e (in), and -1/2 c_e; 0 on an
                      inactive row
    diag, diag_real   (n,) float32: the diagonal of S for tangent and for real features
    w                 (n,) float32, the masses, or None for 1
    h                 the kernel width"""

    def __init__(self, n, n_entries, rowptr, col, edge, coef, coef_real, diag, diag_real, w, h, device):
        self.n, self.n_entries, self.h, self.device = n, n_entries, h, device
        self.rowptr, self.col, self.edge, self.coef, self.coef_real, self.diag, self.diag_real, self.w = \
            rowptr, col, edge, coef, coef_real, diag, diag_real, w
        self._cast = {}

    def operands(self, dtype):
        """(coef, diag, w, scale) for features of `dtype`, in its scalar type, cast once and kept: the complex coefficients and diag
        for complex features, coef_real and diag_real for real ones; w (None without weights) and scale = -1 / w, 0 where w == 0
        (-1 without weights), the row scaling that makes one apply launch the Laplacian or its adjoint."""
        if dtype not in self._cast:
            real = _SCALAR[dtype]
            with _on(self.device):
                if dtype.is_complex:
                    coef, diag = self.coef.to(dtype).contiguous(), self.diag.to(real).contiguous()
                else:
                    coef, diag = self.coef_real.to(real).contiguous(), self.diag_real.to(real).contiguous()
                if self.w is None:
                    w, scale = None, torch.full((self.n,), -1.0, dtype=real, device=self.device)
                else:
                    w = self.w.to(real).contiguous()
                    scale = torch.where(w == 0, torch.zeros_like(w), -1.0 / w).contiguous()
                self._cast[dtype] = (coef, diag, w, scale)
        return self._cast[dtype]

    def to(self, device):
        """The plan on another ROCm device (itself when it is there already)."""
        device = torch.device(device)
        if device.type != 'cuda':
            raise RuntimeError(f'DiffusionPlan.to: a plan lives on a ROCm device, got {device}')
        if device.index is None:
            device = torch.device('cuda', torch.cuda.current_device())
        if device == self.device:
            return self
        mv = lambda t: None if t is None else t.to(device)
        return DiffusionPlan(self.n, self.n_entries, mv(self.rowptr), mv(self.col), mv(self.edge), mv(self.coef), mv(self.coef_real),
                             mv(self.diag), mv(self.diag_real), mv(self.w), self.h, device)

    def __repr__(self):
        return 'DiffusionPlan(n={}, entries={}, h={:.6g}{})'.format(self.n, self.n_entries, self.h, '' if self.w is None else ', weighted')


def _check_h(h, what):
    if h is None:
        return None
    try:
        ok = not isinstance(h, bool) and math.isfinite(float(h)) and 0 < float(h) < 1e30
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: h must be a positive number or None, got {h!r}')
    return float(h)


def diffusion_plan(supp_edges, xp, logMag, n, w=None, h=None):
    """The DiffusionPlan of n samples from the rows [a, b] of supp_edges ((E,2) int64 positions in [0, n), in any order), with
    xp ((E,) complex64, the transport of a row: a's coordinates into b's) and logMag ((E,) float32, its length) -- what
    ComputeLogXPort leaves on data -- and the masses w ((n,) or (n,1) float32, data.w; None for 1).

    A row is active iff a != b, logMag is finite and > 0, xp is finite and both masses are finite and > 0; an inactive row
    keeps its two entries with coefficient 0.  A duplicate row is one more term.  h (a positive number) is the width of the heat
    kernel; None takes fl32(the largest active logMag)^2 / 16, which reads one number back (1 when no row is active).
    A MeshBatch is a union graph: its plan is the plans of its meshes side by side, given the same h.
    One launch (fc_diffusion_coefficients), no atomics: two calls give the same bits.  The plan lives on logMag's device when that
    is a ROCm device, else on the current one."""
    what = 'diffusion_plan'
    if not torch.is_tensor(supp_edges) or supp_edges.dim() != 2 or supp_edges.shape[1] != 2 or supp_edges.dtype != torch.int64:
        raise ValueError(f'{what}: supp_edges must be an (E,2) int64 tensor, got '
                         f'{(tuple(supp_edges.shape), supp_edges.dtype) if torch.is_tensor(supp_edges) else type(supp_edges).__name__}')
    E = int(supp_edges.shape[0])
    for t, name, dt in ((xp, 'xp', torch.complex64), (logMag, 'logMag', torch.float32)):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (E,):
            raise ValueError(f'{what}: {name} must be an ({E},) {dt} tensor, one entry per row of supp_edges, got '
                             f'{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}')
    n = _whole(n, 0, 2 ** 31 - 2, what, 'n', integral_floats=True)
    if 2 * E >= 2 ** 31 - 1:
        raise ValueError(f'{what}: entries are 32-bit indices in the kernel: at most 2^30 - 1 rows, got {E}')
    if w is not None and (not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) not in ((n,), (n, 1))):
        raise ValueError(f'{what}: w must be an ({n},) or ({n},1) float32 tensor or None, got '
                         f'{(tuple(w.shape), w.dtype) if torch.is_tensor(w) else type(w).__name__}')
    h = _check_h(h, what)
    if E and (int(supp_edges.min()) < 0 or int(supp_edges.max()) >= n):
        raise ValueError(f'{what}: supp_edges must hold positions in [0, {n})')
    dev = _device_of(logMag, 'diffusion plans')
    lib = _lib.load()
    with _on(dev):
        r = supp_edges.detach().to(dev)
        a, b = r[:, 0].contiguous(), r[:, 1].contiguous()
        mag = logMag.detach().to(dev).contiguous()
        u = _by_value(xp.detach().to(dev))
        wd = None if w is None else w.detach().to(dev).reshape(-1).contiguous()
        if h is None:
            ur = torch.view_as_real(u)
            active = (a != b) & torch.isfinite(mag) & (mag > 0) & torch.isfinite(ur[:, 0]) & torch.isfinite(ur[:, 1])
            if wd is not None:
                ok = torch.isfinite(wd) & (wd > 0)
                active = active & ok[a] & ok[b]
            top = float(torch.where(active, mag, torch.zeros_like(mag)).max()) if E else 0.0
            h = top * top / 16 if top > 0 else 1.0
        # the merged CSR: row i = its out entries (stable by a), then its in entries (stable by b)
        out, inn = torch.sort(a, stable=True), torch.sort(b, stable=True)
        ends = torch.arange(n + 1, device=dev)
        out_ptr, in_ptr = torch.searchsorted(out.values, ends), torch.searchsorted(inn.values, ends)
        rowptr64 = out_ptr + in_ptr
        slots = torch.arange(E, device=dev)
        at_out = rowptr64[out.values] + (slots - out_ptr[out.values])
        at_in = rowptr64[inn.values] + (out_ptr[inn.values + 1] - out_ptr[inn.values]) + (slots - in_ptr[inn.values])
        col = torch.empty(2 * E, dtype=torch.int32, device=dev)
        edge = torch.empty(2 * E, dtype=torch.int32, device=dev)
        col[at_out], col[at_in] = b[out.indices].to(torch.int32), a[inn.indices].to(torch.int32)
        edge[at_out], edge[at_in] = (-out.indices - 1).to(torch.int32), inn.indices.to(torch.int32)
        rowptr = rowptr64.to(torch.int32)
        coef = torch.empty(2 * E, dtype=torch.complex64, device=dev)
        coef_real = torch.empty(2 * E, dtype=torch.float32, device=dev)
        diag = torch.empty(n, dtype=torch.float32, device=dev)
        diag_real = torch.empty(n, dtype=torch.float32, device=dev)
        _lib.check(lib.fc_diffusion_coefficients(_ptr(rowptr), _ptr(col), _ptr(edge), _ptr(mag), _ptr(u), _ptr(wd), h, n, E, 2 * E, _ptr(coef),
                                                 _ptr(coef_real), _ptr(diag), _ptr(diag_real), _stream()), 'fc_diffusion_coefficients')
        return DiffusionPlan(n, 2 * E, rowptr, col, edge, coef, coef_real, diag, diag_real, wd, h, dev)


def _apply(x, plan, scale_in, scale_out):
    """scale_out * S (scale_in * x) of a checked, contiguous device tensor"""
    C = int(x.shape[1])
    coef, diag, _, _ = plan.operands(x.dtype)
    with _on(x.device):
        y = torch.empty((plan.n, C), dtype=x.dtype, device=x.device)
        _lib.check(_lib.load().fc_diffusion_apply(_ptr(x), _ptr(plan.rowptr), _ptr(plan.col), _ptr(coef), _ptr(diag), _ptr(scale_in),
                                                  _ptr(scale_out), plan.n, plan.n_entries, C, _REAL[_SCALAR[x.dtype]], int(x.dtype.is_complex),
                                                  _ptr(y), _stream()), 'fc_diffusion_apply')
    return y


class _ConnectionLaplacian(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, plan):
        ctx.plan = plan
        x = _by_value(x.detach())
        return _apply(x, plan, None, plan.operands(x.dtype)[3])

    @staticmethod
    def backward(ctx, g):
        if not ctx.needs_input_grad[0]:
            return None, None
        g = _by_value(g.detach())
        return _apply(g, ctx.plan, ctx.plan.operands(g.dtype)[3], None), None          # (-W^-1 S)^H = -S W^-1: the scalings swapped


def _solve(x, t, plan, ptr, host, iters, mode, where, want_lam, want_resid):
    """one launch of fc_diffusion_solve -> (y, lam or None, resid or None)"""
    lib = _lib.load()
    n, C, B = plan.n, int(x.shape[1]), len(host) - 1
    real = _SCALAR[x.dtype]
    dt, cx = _REAL[real], int(x.dtype.is_complex)
    max_rows = max(b - a for a, b in zip(host, host[1:]))
    coef, diag, w, _ = plan.operands(x.dtype)
    with _on(x.device):
        nbytes = lib.fc_diffusion_workspace_bytes(n, B, C, dt, cx, max_rows, where)
        ws = _scratch(nbytes, x.device, 1)
        y = torch.empty((n, C), dtype=x.dtype, device=x.device)
        lam = torch.empty((n, C), dtype=x.dtype, device=x.device) if want_lam else None
        resid = torch.empty((B, C), dtype=real, device=x.device) if want_resid else None
        _lib.check(lib.fc_diffusion_solve(_ptr(x), _ptr(t), _ptr(w), _ptr(diag), _ptr(plan.rowptr), _ptr(plan.col), _ptr(coef), _ptr(ptr), n,
                                          plan.n_entries, B, C, max_rows, dt, cx, iters, mode, where, _ptr(y), _ptr(lam), _ptr(resid), _ptr(ws),
                                          nbytes, _stream()), 'fc_diffusion_solve')
    return y, lam, resid


class _HeatDiffuse(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, plan, ptr, host, iters, where, want_resid):
        xc, tc = _by_value(x.detach()), _by_value(t.detach())
        y, _, resid = _solve(xc, tc, plan, ptr, host, iters, 0, where, False, want_resid)
        ctx.save_for_backward(tc, y)
        ctx.meta = (plan, ptr, host, iters, where)
        if want_resid:
            ctx.mark_non_differentiable(resid)
            return y, resid
        return y

    @staticmethod
    def backward(ctx, gy, *unused):
        need_x, need_t = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_t):
            return (None,) * 8
        plan, ptr, host, iters, where = ctx.meta
        t, y = ctx.saved_tensors
        gy = _by_value(gy.detach().to(y.dtype))
        # lambda = (W + t S)^-1 gy by the same kernel; gx = W lambda; gt = -Re <lambda, S y>
        gx, lam, _ = _solve(gy, t, plan, ptr, host, iters, 1, where, need_t, False)
        gt = None
        if need_t:
            lib = _lib.load()
            C, B, real = int(y.shape[1]), len(host) - 1, _SCALAR[y.dtype]
            sy = _apply(y, plan, None, None)
            with _on(y.device):
                nbytes = (B * C * 8 + 255) // 256 * 256
                ws = _scratch(nbytes, y.device, 1)
                gt = torch.empty((C,), dtype=real, device=y.device)
                _lib.check(lib.fc_diffusion_time_gradient(_ptr(lam), _ptr(sy), _ptr(ptr), plan.n, B, C, _REAL[real], int(y.dtype.is_complex),
                                                          _ptr(gt), _ptr(ws), nbytes, _stream()), 'fc_diffusion_time_gradient')
        return (gx if need_x else None), gt, None, None, None, None, None, None


def _check(x, plan, what):
    if not isinstance(plan, DiffusionPlan):
        raise ValueError(f'{what}: plan must be a DiffusionPlan, got {type(plan).__name__}')
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{what}: x must be an (n, C) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    if x.dtype not in _SCALAR:
        raise TypeError(f'{what}: x is {x.dtype}; complex64 and complex128 (tangent features), float32 and float64 (real features) '
                        'are implemented')
    if not x.is_cuda:
        raise RuntimeError(f'{what}: x is on {x.device}; the operator runs on a ROCm device and has no CPU path')
    if x.device != plan.device:
        raise RuntimeError(f'{what}: x is on {x.device}, the plan on {plan.device}')
    if int(x.shape[0]) != plan.n or int(x.shape[1]) < 1:
        raise ValueError(f'{what}: x must be ({plan.n}, C) with C >= 1 for this plan, got {tuple(x.shape)}')
    if plan.n * int(x.shape[1]) >= 2 ** 40 or int(x.shape[1]) >= 2 ** 29:
        raise ValueError(f'{what}: n * C must stay below 2^40, got {plan.n} x {int(x.shape[1])}')


def connection_laplacian(x, plan):
    """L x = -W^-1 S x (n, C) for x (n, C) on the plan's device: complex64 / complex128 tangent features with the transport phases,
    float32 / float64 real features without.  Per row the entries' terms are added to a zero in entry order, then the diagonal
    term, then the row is scaled by -1 / w (0 where w == 0): one launch, no atomics, the same bits on every run.  Gradient flows
    to x only, and only when x requires one: the same launch with the row scaling moved to the input (S is Hermitian)."""
    _check(x, plan, 'connection_laplacian')
    return _ConnectionLaplacian.apply(x, plan)


def heat_diffuse(x, t, plan, ptr=None, iters=16, return_residual=False, _state=None):
    """y (n, C): per mesh b and channel c the `iters`-step iterate of Jacobi-preconditioned conjugate gradients on

        (W + t_c S) y = W x          started at y = x          (the fixpoint is (I - t_c L)^-1 x; the iterate is what is returned)

    x      (n, C) complex64 / complex128 (tangent features) or float32 / float64 (real features) on the plan's device
    t      (C,) of x's real type, >= 0; t_c = 0 gives y[:, c] = x[:, c] bit for bit; a negative or non-finite t_c makes column c NaN
           and touches nothing else
    ptr    (B+1,) int64 range table (MeshBatch.ptr: no synchronisation), or None: one system of n rows
    iters  an int in [1, 1024]: exactly that many steps, no convergence test, no host read
    return_residual   also return the (B, C) device tensor sqrt(<r, z>) at exit

    One launch (fc_diffusion_solve): a workgroup owns a mesh and 16 bytes of channels through all iterations; vectors are in x's
    precision, the two inner products in double and in a fixed order, so a channel's bits depend on its mesh's rows alone -- not on
    C, on the batch, or on whether the search direction lives in LDS (meshes of at most LDS_ROWS rows) or in the workspace.
    Gradients are those of the exact solve (implicit differentiation): lambda = (W + t S)^-1 gy by the same kernel and the same
    iters from lambda = W^-1 gy, gx = W lambda, gt_c = -Re sum_i conj(lambda[i, c]) (S y)[i, c]; x and t each receive one only
    when they require one.  Both passes may be captured in a StepGraph."""
    what = 'heat_diffuse'
    _check(x, plan, what)
    C, real = int(x.shape[1]), _SCALAR[x.dtype]
    if not torch.is_tensor(t) or t.dtype != real or tuple(t.shape) != (C,):
        raise ValueError(f'{what}: t must be a ({C},) {real} tensor, one time per channel, got '
                         f'{(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}')
    if t.device != x.device:
        raise RuntimeError(f'{what}: t is on {t.device}, x on {x.device}')
    iters = _whole(iters, 1, MAX_ITERS, what, 'iters')
    if _state not in (None, 'workspace'):
        raise ValueError(f"{what}: _state is None or 'workspace', got {_state!r}")
    host = [0, plan.n] if ptr is None else check_ptr(ptr, plan.n, what)
    ptr = None if ptr is None else ptr_on(ptr, host, x.device)
    return _HeatDiffuse.apply(x, t, plan, ptr, host, iters, 0 if _state is None else 1, bool(return_residual))
