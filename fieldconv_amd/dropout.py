"""TangentDropout (csrc/fc_dropout.hip) and the counter-based generator it draws from (csrc/fc_philox.hpp): the functional forms and
the autograd function under fieldconv_amd.nn.TangentDropout, fieldconv_amd.functional.tangent_dropout and
fieldconv_amd.functional.philox_words.

A tangent feature is a complex number in its own sample's frame.  nn.Dropout does not take complex tensors, and on the real view
it drops re and im independently, which rotates the survivor and breaks gauge equivariance.  This op multiplies the whole complex
entry by a REAL mask, which commutes with any change of frames.  The mask comes from Philox4x32-10, a pure function of
(seed, step, stream, entry): there is no generator state to synchronise, a draw can sit inside a StepGraph capture, and
tests/_philox_ref.py restates it bit for bit in numpy.

    T = floor(p * 2^24)                                  (on the host, in double)
    entry e is dropped iff (word >> 8) < T               word e & 3 of block e >> 2 of the draw; an integer comparison
    kept:    y = fl(scale * x), scale = 1 / (1 - p) computed in double and rounded once to x's real type; re and im each
    dropped: y = +0 (+0 +0j) exactly

    mode='element'   e = n C + c: one decision per entry (stream 0)
    mode='channel'   e = b C + c, b the mesh of row n by ptr: one decision per mesh and channel (stream 1)

Features are (N,C) tensors on a ROCm device; there is no CPU or eager path: a CPU tensor raises."""
import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, stream as _stream, whole as _whole
from .pooling import check_ptr, ptr_on

_DTYPES = {torch.float32: (0, 0), torch.float64: (1, 0), torch.complex64: (0, 1), torch.complex128: (1, 1)}          # (fc_dtype, is_complex)
_MODES = {'element': 0, 'channel': 1}
_U64 = 2 ** 64 - 1
_BITS = 24          # a decision compares the top 24 bits of a word: the same bits make a float32 uniform exactly


def drop_threshold(p):
    """T = floor(p * 2^24) in double: an entry is dropped iff (word >> 8) < T"""
    return int(float(p) * float(1 << _BITS))


def keep_scale(p):
    """1 / (1 - p) in double; the kernel rounds it once to the feature's real type"""
    return 1.0 / (1.0 - float(p))


def check_step(step, what, device=None):
    """step as (int, None) or (0, tensor): a Python int >= 0, or a (1,) int64 tensor (on `device`, when that is known)"""
    if torch.is_tensor(step):
        if step.dtype != torch.int64 or tuple(step.shape) != (1,):
            raise ValueError(f'{what}: a tensor step must be a (1,) int64 tensor, got {tuple(step.shape)} {step.dtype}')
        if device is not None and step.device != device:
            raise RuntimeError(f'{what}: step is on {step.device}, the work runs on {device} (the kernel reads the step itself)')
        return 0, step
    return _whole(step, 0, 2 ** 63 - 1, what, 'step'), None


def philox_words(seed, hi, first_block, n_blocks, device=None):
    """(n_blocks, 4) int64 on the device, each entry a 32-bit word: row i holds Philox4x32-10 of the counter
    (lo32(q), hi32(q), lo32(hi), hi32(hi)), q = first_block + i (wrapping at 2^64), under the key (lo32(seed), hi32(seed)).
    seed, hi and first_block are integers in [0, 2^64).  The raw words of the generator, so that it can be pinned on the device."""
    what = 'philox_words'
    seed, hi, first = (_whole(v, 0, _U64, what, n) for v, n in ((seed, 'seed'), (hi, 'hi'), (first_block, 'first_block')))
    n = _whole(n_blocks, 0, 2 ** 40, what, 'n_blocks')
    if not torch.cuda.is_available():
        raise RuntimeError(f'{what}: the generator runs on a ROCm device and none is visible; there is no CPU path')
    dev = torch.device('cuda', torch.cuda.current_device()) if device is None else torch.device(device)
    with _on(dev):
        out = torch.empty((n, 4), dtype=torch.int32, device=dev)
        _lib.check(_lib.load().fc_philox_words(seed, hi, first, n, _ptr(out), _stream()), 'fc_philox_words')
    return out.to(torch.int64) & 0xFFFFFFFF


def _launch(x, ptr, B, threshold, scale, seed, step, step_t, mode):
    """one launch: the mask of the draw (seed, step) applied to a contiguous x"""
    dt, cplx = _DTYPES[x.dtype]
    N, C = int(x.shape[0]), int(x.shape[1])
    with _on(x.device):
        y = torch.empty_like(x)
        _lib.check(_lib.load().fc_dropout(_ptr(x), _ptr(y), N, C, dt, cplx, mode, _ptr(ptr), B, threshold, scale, seed, step, _ptr(step_t),
                                          _stream()), 'fc_dropout')
    return y


class _TangentDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ptr, B, threshold, scale, seed, step, step_t, mode):
        xc = _by_value(x.detach())
        # the step the backward pass draws with: the int, or the device tensor's value of NOW (its owner advances it after the
        # call), cloned before the launch -- only when there will be a backward pass
        need = ctx.needs_input_grad[0]
        kept = step_t.clone() if step_t is not None and need else step_t
        ctx.save_for_backward(ptr, kept if need else None)
        ctx.meta = (B, threshold, scale, seed, step, mode, xc.dtype)
        return _launch(xc, ptr, B, threshold, scale, seed, step, kept, mode)

    @staticmethod
    def backward(ctx, gy):
        if not ctx.needs_input_grad[0]:
            return (None,) * 9
        ptr, kept = ctx.saved_tensors
        B, threshold, scale, seed, step, mode, xdt = ctx.meta
        gy = _by_value(gy.detach().to(xdt))
        return (_launch(gy, ptr, B, threshold, scale, seed, step, kept, mode),) + (None,) * 8


def tangent_dropout(x, p, seed, step, ptr=None, mode='element', training=True):
    """y (N,C) = mask * x / (1 - p) for complex64 / complex128 / float32 / float64 x (N,C) on a ROCm device, the mask REAL: a complex
    entry is kept or dropped whole, so the op commutes with any change of frames.

    p         the drop probability, in [0, 1): entry e is dropped iff (word >> 8) < floor(p * 2^24), an integer comparison
    seed      an integer in [0, 2^64): the generator's key
    step      the draw number (its low 32 bits): a Python int >= 0, or a (1,) int64 tensor on x's device, which the kernel reads
              itself -- no synchronisation, and a graph replay sees the tensor's current value
    ptr       (B+1,) int64 range table (MeshBatch.ptr: no synchronisation), or None: one mesh; read in mode='channel' only
    mode      'element': one decision per entry, e = n C + c.  'channel': one per mesh and channel, e = b C + c -- a whole feature
              channel of a mesh is silenced; every row of a mesh shares its mesh's decision.  Empty meshes are allowed.
    training  False returns x itself (after the argument checks)

    A kept entry is fl(scale * x) with scale = 1 / (1 - p) computed in double and rounded once to x's real type, re and im each; a
    dropped entry is exactly +0.  p = 0 gives a new tensor with x's bits.  The result is a function of (seed, step, mode, e) alone:
    the same bits on every run, whatever the launch geometry (tests/_philox_ref.py restates it in numpy).  One native launch
    forward and one backward -- the same entry point on the gradient, with the step of the forward pass; the mask is never
    stored.  Only x receives a gradient.  Non-contiguous x is made contiguous."""
    what = 'tangent_dropout'
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{what}: x must be an (N,C) tensor, got {tuple(x.shape) if torch.is_tensor(x) else type(x).__name__}')
    if x.dtype not in _DTYPES:
        raise TypeError(f'{what}: x is {x.dtype}; complex64, complex128, float32 and float64 are implemented')
    N, C = int(x.shape[0]), int(x.shape[1])
    if C < 1 or C > 64 * 65535:
        raise ValueError(f'{what}: between 1 and {64 * 65535} channels, got {C}')
    try:
        p_ok = not isinstance(p, bool) and 0.0 <= float(p) < 1.0
    except (TypeError, ValueError):
        p_ok = False
    if not p_ok:
        raise ValueError(f'{what}: p must be a number in [0, 1), got {p!r}')
    if mode not in _MODES:
        raise ValueError(f"{what}: mode must be 'element' or 'channel', got {mode!r}")
    if not isinstance(training, bool):
        raise ValueError(f'{what}: training must be True or False, got {training!r}')
    seed = _whole(seed, 0, _U64, what, 'seed')
    step, step_t = check_step(step, what)
    host = [0, N] if ptr is None else check_ptr(ptr, N, what)          # (checked in both modes, read in 'channel' only)
    if N + 64 * (len(host) - 1) >= 2 ** 31 - 1:
        raise ValueError(f'{what}: rows + 64 * meshes must stay below 2^31')
    if not training:
        return x
    if not x.is_cuda:          # (after the argument checks: those need no device)
        raise RuntimeError(f'{what}: x is on {x.device}; fieldconv_amd dropout runs on a ROCm device and has no CPU path')
    check_step(step_t if step_t is not None else step, what, x.device)
    ptr = None if ptr is None else ptr_on(ptr, host, x.device)
    return _TangentDropout.apply(x, ptr, len(host) - 1, drop_threshold(p), keep_scale(p), seed, step, step_t, _MODES[mode])
