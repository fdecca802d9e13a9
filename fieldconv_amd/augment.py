"""Per-mesh augmentation of a mini-batch of meshes (csrc/fc_augment.hip): one random similarity per mesh, drawn on the device from
the counter-based generator (csrc/fc_philox.hpp, stream 2), and its application to every mesh's vertices in one launch -- the
functional forms under fieldconv_amd.transforms.RandomMeshAffine.

The reference's notebooks wrap their datasets in Compose((Center() | RandomScale((0.85, 1.15)), RandomRotate(45, axis=0),
RandomRotate(45, axis=1), RandomRotate(45, axis=2))): host transforms of one mesh.  A batch needs its own centre, scale and
rotation per mesh; a loop over batch.mesh(b) would undo what the batched preprocessing bought.

    mesh b uses block q = b of the draw (seed, step), u_k = (word k >> 8) * 2^-24:
    s   = lo + (hi - lo) * u_0                      (1, and u_0 unused, without a scale range)
    a_k = (2 * u_{k+1} - 1) * degrees[k]            the angle about axis k, in degrees
    M   = s Rz(r_2) Ry(r_1) Rx(r_0),  r_k = a_k * fl32(pi / 180)       for column vectors: scale, rotate about axis 0, then 1, then 2
    out = M (p - t)

Positions are float32 tensors on a ROCm device; there is no CPU or eager path: a CPU tensor raises."""
import torch

from . import _lib
from ._launch import device_of as _device_of, on as _on, ptr as _ptr, stream as _stream, whole as _whole
from .dropout import check_step
from .pooling import check_ptr, ptr_on

_U64 = 2 ** 64 - 1


def check_ranges(scale, degrees, what):
    """-> (has_scale, lo, hi, (d0, d1, d2)) as floats; ValueError for anything else"""
    try:
        degs = tuple(float(d) for d in ((degrees,) * 3 if isinstance(degrees, (int, float)) and not isinstance(degrees, bool) else degrees))
        ok = len(degs) == 3 and all(0.0 <= d <= 360.0 for d in degs)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: degrees must be one number or three, each in [0, 360], got {degrees!r}')
    if scale is None:
        return 0, 1.0, 1.0, degs
    try:
        lo, hi = (float(v) for v in scale)
        ok = 0.0 < lo <= hi < float('inf')
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: scale must be None or (lo, hi) with 0 < lo <= hi, got {scale!r}')
    return 1, lo, hi, degs


def random_mesh_affine(B, seed, step, scale=None, degrees=(45, 45, 45), device=None):
    """(params (B,4), M (B,3,3)) float32 on the device, from one launch: params[b] = (s, a_0, a_1, a_2), the scale and the three
    angles in degrees of mesh b, and M[b] = s Rz(r_2) Ry(r_1) Rx(r_0) with r_k = a_k * fl32(pi / 180).

    seed      an integer in [0, 2^64)
    step      the draw number: a Python int >= 0, or a (1,) int64 device tensor that the kernel reads itself
    scale     None (s = 1) or (lo, hi): s = lo + (hi - lo) * u_0
    degrees   the largest angle about each axis: a_k = (2 * u_{k+1} - 1) * degrees[k]
    device    where to draw; a tensor step's device, else the current ROCm device

    params is a chain of float32 operations each rounded on its own, so numpy gives the same bits (tests/_philox_ref.py); M goes
    through the device library's sinf and cosf and is accurate to a few units in the last place, not bit-exact."""
    what = 'random_mesh_affine'
    B = _whole(B, 1, 2 ** 31 - 1, what, 'B')
    seed = _whole(seed, 0, _U64, what, 'seed')
    has_scale, lo, hi, degs = check_ranges(scale, degrees, what)
    step, step_t = check_step(step, what)
    if device is not None:
        dev = torch.device(device)
    elif step_t is not None and step_t.is_cuda:
        dev = step_t.device
    else:
        dev = _device_of(torch.empty(0), 'augmentations')
    if dev.type != 'cuda':
        raise RuntimeError(f'{what}: {dev} is no ROCm device; fieldconv_amd augmentation has no CPU path')
    check_step(step_t if step_t is not None else step, what, dev)
    with _on(dev):
        params = torch.empty((B, 4), dtype=torch.float32, device=dev)
        M = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().fc_mesh_affine_draw(B, seed, step, _ptr(step_t), has_scale, lo, hi, degs[0], degs[1], degs[2], _ptr(params),
                                                   _ptr(M), _stream()), 'fc_mesh_affine_draw')
    return params, M


def mesh_affine(pos, pos_ptr, M, t=None, index=None):
    """out (R,3) float32: row r is M[b] (pos[v] - t[b]) for the vertex v = index[r] (v = r, R = V, without index) of the mesh b
    that owns v by pos_ptr; out_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2, every operation rounded on its own in float32.

    pos       (V,3) float32 on a ROCm device
    pos_ptr   (B+1,) int64 range table of the vertices (MeshBatch.pos_ptr: no synchronisation)
    M         (B,3,3) float32;  t (B,3) float32 or None (nothing subtracted)
    index     (R,) int64 or None; an entry outside [0, V) gives a row of NaN and reads nothing

    A new tensor: pos is not written.  One launch, no workspace.  No gradient flows (an augmentation of the input)."""
    what = 'mesh_affine'
    if not torch.is_tensor(pos) or pos.dim() != 2 or pos.shape[1] != 3 or pos.dtype != torch.float32:
        raise ValueError(f'{what}: pos must be a (V,3) float32 tensor, got '
                         f'{(tuple(pos.shape), pos.dtype) if torch.is_tensor(pos) else type(pos).__name__}')
    V = int(pos.shape[0])
    host = check_ptr(pos_ptr, V, what, 'pos_ptr')
    B = len(host) - 1
    if V >= 2 ** 31 - 1:
        raise ValueError(f'{what}: fewer than 2^31 - 1 vertices')
    if not torch.is_tensor(M) or M.dtype != torch.float32 or tuple(M.shape) != (B, 3, 3):
        raise ValueError(f'{what}: M must be a ({B},3,3) float32 tensor, got {(tuple(M.shape), M.dtype) if torch.is_tensor(M) else type(M).__name__}')
    if t is not None and (not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != (B, 3)):
        raise ValueError(f'{what}: t must be a ({B},3) float32 tensor or None, got {(tuple(t.shape), t.dtype) if torch.is_tensor(t) else type(t).__name__}')
    if index is not None and (not torch.is_tensor(index) or index.dtype != torch.int64 or index.dim() != 1):
        raise ValueError(f'{what}: index must be an (R,) int64 tensor or None, got '
                         f'{(tuple(index.shape), index.dtype) if torch.is_tensor(index) else type(index).__name__}')
    if not pos.is_cuda:          # (after the argument checks: those need no device)
        raise RuntimeError(f'{what}: pos is on {pos.device}; fieldconv_amd augmentation runs on a ROCm device and has no CPU path')
    for name, v in (('M', M), ('t', t), ('index', index)):
        if v is not None and v.device != pos.device:
            raise RuntimeError(f'{what}: {name} is on {v.device}, pos on {pos.device}')
    dev = pos.device
    pc, Mc = pos.detach().contiguous(), M.detach().contiguous()
    tc = None if t is None else t.detach().contiguous()
    ic = None if index is None else index.contiguous()
    R = V if ic is None else int(ic.shape[0])
    with _on(dev):
        ptr = ptr_on(pos_ptr, host, dev)
        out = torch.empty((R, 3), dtype=torch.float32, device=dev)
        _lib.check(_lib.load().fc_mesh_affine_apply(_ptr(pc), _ptr(ptr), B, V, _ptr(Mc), _ptr(tc), _ptr(ic), R, _ptr(out), _stream()),
                   'fc_mesh_affine_apply')
    return out
