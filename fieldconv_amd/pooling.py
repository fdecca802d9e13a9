"""Per-mesh pooling over a mini-batch of meshes (csrc/fc_segment.hip): the functional forms and the autograd function under
fieldconv_amd.nn.MeshPool and fieldconv_amd.functional.mesh_mean; and mesh_max, the max read-out by magnitude under
fieldconv_amd.nn.MeshMaxPool (csrc/fc_maxpool.hip).

A mini-batch is a disjoint union: mesh b owns the rows ptr[b] .. ptr[b+1] - 1 of every per-vertex tensor (ptr: (B+1,) int64,
ascending, ptr[0] = 0, ptr[-1] = N; MeshBatch.ptr).  Features are (N,C) tensors on a ROCm device; there is no CPU or eager
path: a CPU tensor raises.  ptr may live on the host or on the device.  Its VALUES are checked on the host before anything
is launched: a host ptr costs nothing, a MeshBatch's ptr carries its host copy along, and any other device ptr is read back
once -- the one synchronisation -- and remembered for as long as the tensor is not modified."""
import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream

_DTYPES = {torch.float32: 0, torch.float64: 1, torch.complex64: 0, torch.complex128: 1}
_REAL = {torch.complex64: torch.float32, torch.complex128: torch.float64}
_REDUCE = {'mean': 0, 'sum': 1}


def tag_ptr(ptr, host):
    """Attach the host copy of a range table to its tensor (MeshBatch does, for the tables it builds from shapes)."""
    ptr._fc_ptr_host = (ptr._version, [int(v) for v in host])
    return ptr


def ptr_host(ptr, what, name='ptr'):
    """The entries of a (B+1,) int64 range table as Python ints, without a synchronisation where the tensor is on the host or
    carries its host copy (tag_ptr); otherwise read back once and kept with the tensor."""
    if not torch.is_tensor(ptr) or ptr.dim() != 1 or ptr.dtype != torch.int64 or ptr.numel() < 2:
        raise ValueError(f'{what}: {name} must be a (B+1,) int64 tensor with B >= 1, got '
                         f'{(tuple(ptr.shape), ptr.dtype) if torch.is_tensor(ptr) else type(ptr).__name__}')
    memo = getattr(ptr, '_fc_ptr_host', None)
    if memo is not None and memo[0] == ptr._version and len(memo[1]) == ptr.numel():
        return memo[1]
    host = ptr.tolist()
    tag_ptr(ptr, host)
    return host


def check_ptr(ptr, n_rows, what, name='ptr'):
    """-> the table's entries as Python ints; ValueError unless 0 = ptr[0] <= ptr[1] <= ... <= ptr[B] = n_rows."""
    host = ptr_host(ptr, what, name)
    if host[0] != 0 or host[-1] != n_rows:
        raise ValueError(f'{what}: {name} must run from 0 to the number of rows ({n_rows}), got {name}[0] = {host[0]}, {name}[-1] = {host[-1]}')
    if any(b < a for a, b in zip(host, host[1:])):
        raise ValueError(f'{what}: {name} must be ascending (a mesh is a contiguous range of rows)')
    return host


def ptr_on(ptr, host, device):
    """The table as a contiguous int64 tensor on `device` (its host copy travels with it)."""
    if ptr.device == device and ptr.is_contiguous():
        return ptr
    return tag_ptr(ptr.to(device).contiguous(), host)


def per_mesh(value, B, what, name):
    """An argument given once for all B meshes, or as a list, tuple or tensor with one entry per mesh -> the list of B entries."""
    vals = list(value) if isinstance(value, (list, tuple)) or torch.is_tensor(value) else [value] * B
    if len(vals) != B:
        raise ValueError(f'{what}: {name} must be one integer or one per mesh ({B}), got {len(vals)}')
    return vals


class _MeshPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, reduce, soft_abs):
        lib = _lib.load()
        xc = _by_value(x.detach())
        N, C, B = int(xc.shape[0]), int(xc.shape[1]), int(ptr.numel()) - 1
        dev, dt = xc.device, _DTYPES[xc.dtype]
        rdt = _REAL[xc.dtype] if soft_abs else xc.dtype
        with _on(dev):
            nbytes = lib.fc_segment_pool_workspace_bytes(N, B, C, dt)
            ws = _scratch(nbytes, dev, 1)
            out = torch.empty((B, C), dtype=rdt, device=dev)
            fn, name = (lib.fc_segment_pool_soft_abs_forward, 'fc_segment_pool_soft_abs_forward') if soft_abs else \
                       (lib.fc_segment_pool_forward, 'fc_segment_pool_forward')
            _lib.check(fn(_ptr(xc), _ptr(ptr), N, B, C, dt, reduce, _ptr(out), _ptr(ws), nbytes, _stream()), name)
        ctx.save_for_backward(xc if soft_abs else None, ptr)
        ctx.meta = (N, C, B, dt, reduce, soft_abs, xc.dtype)
        return out

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, ptr = ctx.saved_tensors
        N, C, B, dt, reduce, soft_abs, xdt = ctx.meta
        dev = ptr.device
        with _on(dev):
            g = _by_value(g.detach().to(_REAL[xdt] if soft_abs else xdt))
            gx = torch.empty((N, C), dtype=xdt, device=dev)
            if soft_abs:
                _lib.check(lib.fc_segment_pool_soft_abs_backward(_ptr(x), _ptr(g), _ptr(ptr), N, B, C, dt, reduce, _ptr(gx), _stream()),
                           'fc_segment_pool_soft_abs_backward')
            else:
                _lib.check(lib.fc_segment_pool_backward(_ptr(g), _ptr(ptr), N, B, C, dt, reduce, _ptr(gx), _stream()),
                           'fc_segment_pool_backward')
        return gx, None, None, None


def mesh_pool(x, ptr, reduce='mean', soft_abs=True, what='mesh_pool'):
    """(B,C) real tensor: out[b,c] = mean (or sum) over the rows n of mesh b of softAbs(x[n,c]) for complex64 / complex128 x (N,C)
    (soft_abs=True: |x| outside the origin box, 0 inside, reference utils/field.py:29-37 -- the classification read-out
    mean(softAbs(x), dim=0) per mesh, |x| never written out), or of x[n,c] itself for float32 / float64 x (soft_abs=False).
    An empty mesh gives 0.  Sums run in the input's precision in a fixed order (include/fieldconv_hip.h): the same bits on
    every run.  Gradient flows to x."""
    if reduce not in _REDUCE:
        raise ValueError(f"{what}: reduce must be 'mean' or 'sum', got {reduce!r}")
    want = (torch.complex64, torch.complex128) if soft_abs else (torch.float32, torch.float64)
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in want:
        raise ValueError(f'{what}: x must be an (N,C) ' + ('complex64 or complex128' if soft_abs else 'float32 or float64') +
                         f' tensor, got {(tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__}')
    if not x.is_cuda:
        raise RuntimeError(f'{what}: x is on {x.device}; fieldconv_amd pooling runs on a ROCm device and has no CPU path')
    N, C = int(x.shape[0]), int(x.shape[1])
    if C < 1 or C > 64 * 65535:
        raise ValueError(f'{what}: between 1 and {64 * 65535} channels, got {C}')
    host = check_ptr(ptr, N, what)
    if N + 64 * (len(host) - 1) >= 2 ** 31 - 1:
        raise ValueError(f'{what}: rows + 64 * meshes must stay below 2^31')
    return _MeshPool.apply(x, ptr_on(ptr, host, x.device), _REDUCE[reduce], bool(soft_abs))


class _MeshMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr):
        lib = _lib.load()
        xc = _by_value(x.detach())
        N, C, B = int(xc.shape[0]), int(xc.shape[1]), int(ptr.numel()) - 1
        dev, dt, cplx = xc.device, _DTYPES[xc.dtype], int(xc.is_complex())
        rdt = _REAL[xc.dtype] if cplx else xc.dtype
        with _on(dev):
            slots = N // 64 + B          # the chunk slots of csrc/fc_segment.hpp: room for every mesh's chunks, whatever ptr holds
            pkey = torch.empty((slots, C), dtype=rdt, device=dev)
            prow = torch.empty((slots, C), dtype=torch.int32, device=dev)
            out = torch.empty((B, C), dtype=rdt, device=dev)
            index = torch.empty((B, C), dtype=torch.int32, device=dev)
            _lib.check(lib.fc_segment_max_forward(_ptr(xc), _ptr(ptr), N, B, C, dt, cplx, _ptr(out), _ptr(index), _ptr(pkey), _ptr(prow),
                                                  _stream()), 'fc_segment_max_forward')
        ctx.save_for_backward(xc if cplx else None, ptr, index)
        ctx.meta = (N, C, B, dt, cplx, xc.dtype)
        ctx.mark_non_differentiable(index)
        return out, index

    @staticmethod
    def backward(ctx, g, _):
        lib = _lib.load()
        x, ptr, index = ctx.saved_tensors
        N, C, B, dt, cplx, xdt = ctx.meta
        dev = ptr.device
        with _on(dev):
            g = _by_value(g.detach().to(_REAL[xdt] if cplx else xdt))
            gx = torch.empty((N, C), dtype=xdt, device=dev)
            _lib.check(lib.fc_segment_max_backward(_ptr(x), _ptr(g), _ptr(index), _ptr(ptr), N, B, C, dt, cplx, _ptr(gx), _stream()),
                       'fc_segment_max_backward')
        return gx, None


def mesh_max(x, ptr, soft_abs=True, return_indices=False, what='mesh_max'):
    """(B,C) real tensor: per mesh and channel the ONE row of largest key (csrc/fc_maxpool.hip, include/fieldconv_hip.h).
      key      complex64 / complex128 x (N,C), soft_abs=True (the only mode for complex input): k = fl(fl(re * re) + fl(im * im)) in
               x's scalar type, every operation rounded on its own -- the squared magnitude, which does not depend on the row's
               frame.  float32 / float64 x, soft_abs=False: k = x itself, a plain max.
      winner   the row n* of mesh b (rows ptr[b] .. ptr[b+1] - 1) with the largest key; ties go to the smallest row.  NaN is outside
               the contract.
      value    complex: out[b,c] = softAbs(x[n*,c]): |x| outside the origin box, 0 inside (reference utils/field.py:29-37); |x| is
               never written per row.  It is the softAbs of the entry of largest key: softAbs is not strictly monotone in |x| at the
               corner of the origin box, so another row may have a larger softAbs.  Real: x[n*,c], bit for bit.
    An empty mesh gives 0, index -1 and no gradient.  With return_indices also the (B,C) int64 winning rows.  Two launches
    forward (partial winners per chunk of 64 rows, then one combination per mesh, both in the (key, row) order: the result is a
    plain argmax whatever the chunking), one backward, no atomics: the same bits on every run and for a mesh alone or inside a
    batch.  Gradient flows to x: g[b,c] * x / |x| outside the origin box (0 inside) at the winner, g[b,c] for real x, and exactly 0
    at every other row.  Checks are mesh_pool's; a MeshBatch's ptr costs no synchronisation."""
    if not isinstance(soft_abs, bool) or not isinstance(return_indices, bool):
        raise ValueError(f'{what}: soft_abs and return_indices must be True or False, got {soft_abs!r} and {return_indices!r}')
    want = (torch.complex64, torch.complex128) if soft_abs else (torch.float32, torch.float64)
    if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in want:
        raise ValueError(f'{what}: x must be an (N,C) ' + ('complex64 or complex128' if soft_abs else 'float32 or float64') +
                         f' tensor, got {(tuple(x.shape), x.dtype) if torch.is_tensor(x) else type(x).__name__}')
    if not x.is_cuda:
        raise RuntimeError(f'{what}: x is on {x.device}; fieldconv_amd pooling runs on a ROCm device and has no CPU path')
    N, C = int(x.shape[0]), int(x.shape[1])
    if C < 1 or C > 64 * 65535:
        raise ValueError(f'{what}: between 1 and {64 * 65535} channels, got {C}')
    host = check_ptr(ptr, N, what)
    if N + 64 * (len(host) - 1) >= 2 ** 31 - 1:
        raise ValueError(f'{what}: rows + 64 * meshes must stay below 2^31')
    out, index = _MeshMax.apply(x, ptr_on(ptr, host, x.device))
    return (out, index.to(torch.int64)) if return_indices else out


def mesh_mean(values, ptr):
    """(B,C): the mean over each mesh's rows of a real (N,C) float32 / float64 device tensor; (N,) input gives (B,).  With a
    per-vertex loss this is the reference's batch_step arithmetic in one step:
        mesh_mean(cross_entropy(logits, y, reduction='none')[:, None], batch.ptr).mean()  ==  sum_b CE_b / B"""
    if torch.is_tensor(values) and values.dim() == 1:
        return mesh_pool(values[:, None], ptr, 'mean', False, 'mesh_mean')[:, 0]
    return mesh_pool(values, ptr, 'mean', False, 'mesh_mean')
