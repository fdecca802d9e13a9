"""TangentNorm (csrc/fc_norm.hip): per-mesh normalisation of tangent features, the functional form and the autograd function under
fieldconv_amd.nn.TangentNorm and fieldconv_amd.functional.tangent_norm.

A tangent feature is a complex number in its own sample's frame.  Subtracting a mean over samples mixes frames, and the stock
normalisers on the real view treat re and im as independent channels; both break gauge equivariance.  This layer scales every
channel of every mesh by the reciprocal root of its (weighted) mean squared magnitude and does nothing else, so it commutes with
any change of frames:

    W[b]    = sum_{n in b} w[n]
    m[b,c]  = sum_{n in b} w[n] |x[n,c]|^2 / W[b]          (0 where W[b] == 0, and for an empty mesh)
    r[b,c]  = 1 / sqrt(m[b,c] + eps)
    y[n,c]  = gain[c] r[b,c] x[n,c]

Features are (N,C) complex tensors on a ROCm device; there is no CPU or eager path: a CPU tensor raises.  The range table ptr is
handled as fieldconv_amd.pooling handles it: a MeshBatch's ptr costs no synchronisation."""
import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream
from .pooling import check_ptr, ptr_on, tag_ptr

_DTYPES = {torch.complex64: 0, torch.complex128: 1}
_REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}


class _TangentNorm(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, gain, ptr, w, eps):
        lib = _lib.load()
        xc = _by_value(x.detach())
        N, C, B = int(xc.shape[0]), int(xc.shape[1]), int(ptr.numel()) - 1
        dev, dt, real = xc.device, _DTYPES[xc.dtype], _REAL[xc.dtype]
        gc = None if gain is None else _by_value(gain.detach().reshape(-1))
        wc = None if w is None else _by_value(w.detach().reshape(-1))
        with _on(dev):
            nbytes = lib.fc_tangent_norm_workspace_bytes(N, B, C, dt)
            ws = _scratch(nbytes, dev, 1)
            y = torch.empty((N, C), dtype=xc.dtype, device=dev)
            r = torch.empty((B, C), dtype=real, device=dev)
            _lib.check(lib.fc_tangent_norm_forward(_ptr(xc), _ptr(wc), _ptr(ptr), _ptr(gc), N, B, C, dt, float(eps), _ptr(y), _ptr(r), _ptr(ws),
                                                   nbytes, _stream()), 'fc_tangent_norm_forward')
        ctx.save_for_backward(xc, gc, ptr, wc, r)
        ctx.meta = (N, C, B, dt, None if gain is None else tuple(gain.shape))
        return y

    @staticmethod
    def backward(ctx, gy):
        need_x, need_gain = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if not (need_x or need_gain):
            return None, None, None, None, None
        lib = _lib.load()
        x, gain, ptr, w, r = ctx.saved_tensors
        N, C, B, dt, gain_shape = ctx.meta
        dev = x.device
        with _on(dev):
            gy = _by_value(gy.detach().to(x.dtype))
            nbytes = lib.fc_tangent_norm_workspace_bytes(N, B, C, dt)
            ws = _scratch(nbytes, dev, 1)
            gx = torch.empty((N, C), dtype=x.dtype, device=dev) if need_x else None
            gg = torch.empty((C,), dtype=r.dtype, device=dev) if need_gain else None
            if N > 0 or need_gain:
                _lib.check(lib.fc_tangent_norm_backward(_ptr(x), _ptr(w), _ptr(ptr), _ptr(gain), _ptr(r), _ptr(gy), N, B, C, dt, _ptr(gx), _ptr(gg),
                                                        _ptr(ws), nbytes, _stream()), 'fc_tangent_norm_backward')
        return gx, (gg.reshape(gain_shape) if need_gain else None), None, None, None


def whole_ptr(n_rows, device):
    """The range table [0, n_rows] of one mesh on `device`, with its host copy attached: built by device fills from the shape
    alone, so it costs no synchronisation and may sit inside a stream capture."""
    ptr = torch.full((2,), int(n_rows), dtype=torch.int64, device=device)
    ptr[:1].zero_()
    return tag_ptr(ptr, [0, int(n_rows)])


def tangent_norm(x, gain=None, ptr=None, w=None, eps=1e-5):
    """y (N,C) = gain[c] * r[b,c] * x[n,c] for complex64 / complex128 x (N,C) on a ROCm device, with r[b,c] = 1 / sqrt(m[b,c] + eps)
    and m[b,c] the w-weighted mean of |x[n,c]|^2 over the rows n of mesh b (0 for an empty mesh and where the mesh's weights sum
    to 0).  No mean is subtracted: only magnitudes are touched, so the op commutes with any change of frames.

    gain  (1,C) or (C,) real of x's real dtype, or None for 1
    ptr   (B+1,) int64 range table (MeshBatch.ptr: no synchronisation), or None: the whole tensor is one mesh
    w     (N,) or (N,1) real of x's real dtype, non-negative (data.w, the integration weights), or None for 1
    eps   >= 0; with eps = 0 an all-zero channel of a mesh gives NaN

    All arithmetic runs in x's precision; magnitudes whose squares leave the float32 range (|x| beyond about 1.8e19, or so small
    that |x|^2 underflows) are outside the contract for complex64.  Sums run in a fixed order that depends on a mesh's own row
    count and C only (include/fieldconv_hip.h): the same bits on every run, and for a mesh alone or inside a batch.  Three native
    launches forward, at most four backward.  Gradient flows to x and gain, to each only when it requires one; ptr, w and eps
    never receive one.  Non-contiguous x is made contiguous."""
    what = 'tangent_norm'
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{what}: x must be an (N,C) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    if x.dtype not in _DTYPES:
        raise TypeError(f'{what}: x is {x.dtype}; complex64 and complex128 are implemented (tangent features are complex)')
    N, C = int(x.shape[0]), int(x.shape[1])
    real = _REAL[x.dtype]
    if C < 1 or C > 64 * 65535:
        raise ValueError(f'{what}: between 1 and {64 * 65535} channels, got {C}')
    try:
        eps_ok = not isinstance(eps, bool) and float(eps) >= 0
    except (TypeError, ValueError):
        eps_ok = False
    if not eps_ok:
        raise ValueError(f'{what}: eps must be a number >= 0, got {eps!r}')
    if gain is not None:
        if not torch.is_tensor(gain) or gain.dtype != real or tuple(gain.shape) not in ((1, C), (C,)):
            raise ValueError(f'{what}: gain must be a (1,{C}) or ({C},) {real} tensor or None, got '
                             f'{(tuple(gain.shape), gain.dtype) if torch.is_tensor(gain) else type(gain).__name__}')
    if w is not None:
        if not torch.is_tensor(w) or w.dtype != real or tuple(w.shape) not in ((N,), (N, 1)):
            raise ValueError(f'{what}: w must be an ({N},) or ({N},1) {real} tensor or None, got '
                             f'{(tuple(w.shape), w.dtype) if torch.is_tensor(w) else type(w).__name__}')
    host = [0, N] if ptr is None else check_ptr(ptr, N, what)
    if N + 64 * (len(host) - 1) >= 2 ** 31 - 1:
        raise ValueError(f'{what}: rows + 64 * meshes must stay below 2^31')
    if not x.is_cuda:          # (after the argument checks: those need no device)
        raise RuntimeError(f'{what}: x is on {x.device}; fieldconv_amd normalisation runs on a ROCm device and has no CPU path')
    for name, t in (('gain', gain), ('w', w)):
        if t is not None and t.device != x.device:
            raise RuntimeError(f'{what}: {name} is on {t.device}, x on {x.device}')
    ptr = whole_ptr(N, x.device) if ptr is None else ptr_on(ptr, host, x.device)
    return _TangentNorm.apply(x, gain, ptr, w, float(eps))
