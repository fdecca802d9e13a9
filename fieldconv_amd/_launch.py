"""The host side of a native launch, each idiom once: raw pointers, the current stream, the device guard, workspaces, the device
a CPU input is computed on, and the integer check of a Python argument.  A leaf module: every operator module binds what it
needs from here (under a leading underscore), none borrows it from a sibling."""
import ctypes
import math
import operator

import torch

_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None)
_cur_device = getattr(torch._C, '_cuda_getDevice', None)


def stream():
    """The current HIP stream of the current device as a raw pointer.  torch.cuda.current_stream() costs ~10 us of
    Python per call -- with ~25 launches per network forward that was a quarter of the host's enqueue time."""
    if _raw_stream is not None and _cur_device is not None:
        return ctypes.c_void_p(_raw_stream(_cur_device()))
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


NO_GUARD = _NoGuard()


def on(device):
    """Device guard for a launch; free when `device` already is the current one (the usual case)."""
    if _cur_device is not None and device.index is not None and _cur_device() == device.index:
        return NO_GUARD
    return torch.cuda.device(device)


def _p(t):
    return ctypes.c_void_p(t.data_ptr())


def _dp(t):
    """data pointer of an optional tensor (None: NULL) for a struct field"""
    return t.data_ptr() if t is not None else None


def _po(t):
    """_p of an optional tensor (None: NULL)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def ptr(t):
    """_po that also gives NULL for an empty tensor, whatever address its storage has (a slice of a live buffer, say)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def by_value(t, align=0):
    """The tensor a launch may take the pointer of in place of `t`: contiguous, lazy conjugate and negative bits resolved -- the kernels
    read raw memory, and a bare .contiguous() hands a lazily conjugated or negated tensor back as it is.  A plain contiguous tensor is
    returned ITSELF (no copy, no new tensor object); everything else is copied.  align: the bytes a kernel's vector loads assume of
    the base address where that is more than the element size (a contiguous view may start anywhere in its storage): such a view is
    copied too."""
    t = t.resolve_conj().resolve_neg().contiguous()
    if align and t.data_ptr() % align:
        t = t.clone()
    return t


def scratch(nbytes, device, floor=0):
    """Device scratch of `nbytes` bytes (uint8), the ONE place workspaces are allocated.  What a zero-byte request gives follows the
    entry point: floor=0 an empty tensor (its pointer is NULL), floor=1 a live one-byte buffer (the block-level entry points),
    floor=None no tensor at all (fc_forward_*, fc_cgemm: _po(None) is NULL)."""
    if floor is None:
        if not nbytes:
            return None
        floor = 0
    return torch.empty(max(int(nbytes), floor), dtype=torch.uint8, device=device)


def carve(shapes, device, zero=False, extra=None):
    """One flat float32 buffer and a view of it per shape, pieces 16-byte aligned (None entries stay None and take no room); with
    `extra`, that many floats behind the pieces come last, flat.  Everything returned shares ONE storage."""
    counts = [math.prod(shp) for shp in shapes if shp is not None]
    sizes = [(n + 3) // 4 * 4 for n in counts]
    flat = (torch.zeros if zero else torch.empty)(sum(sizes) + (extra or 0), dtype=torch.float32, device=device)
    parts = iter(flat.split(sizes if extra is None else sizes + [extra]))
    counts = iter(counts)
    out = []
    for shp in shapes:
        if shp is None:
            out.append(None)
        else:
            n = next(counts)
            out.append(next(parts)[:n].view(shp) if n % 4 else next(parts).view(shp))
    if extra is not None:
        out.append(next(parts))
    return out


def device_of(t, family):
    """The ROCm device the work on `t` runs on: its own, or the current one for a CPU tensor.  `family` names the results in the
    error ('geodesics', 'support graphs')."""
    if t.is_cuda:
        return t.device
    if not torch.cuda.is_available():
        raise RuntimeError(f'fieldconv_amd {family} are computed on a ROCm device and none is visible; there is no CPU path')
    return torch.device('cuda', torch.cuda.current_device())


def whole(v, lo, hi, what, name, where='', integral_floats=False):
    """v as an int in [lo, hi], or ValueError.  A bool never counts; anything with __index__ does (numpy integers, 0-dim integer
    tensors); integral_floats also admits what equals its own int(): 3.0, not 1.5."""
    try:
        if isinstance(v, bool):
            n = None
        elif integral_floats:
            n = int(v) if int(v) == v else None
        else:
            n = operator.index(v)
    except (TypeError, ValueError, OverflowError):
        n = None
    if n is None or not lo <= n <= hi:
        raise ValueError(f'{what}: {name}{where} must be an integer in [{lo}, {hi}], got {v!r}')
    return n
