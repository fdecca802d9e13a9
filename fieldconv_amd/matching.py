"""Descriptor matching on the device (csrc/fc_match.hip): which rows of xS are nearest to each row of xT.

Features are real (N,C) float32 or float64 tensors on a ROCm device, as in fieldconv_amd.losses; pairs are rows
[row of xT, row of xS].  The distance is the losses' d2, bit for bit (one definition in the library), so a match and its
TwinEval verdict cannot disagree at a threshold, and the N_T x N_S matrix never exists: memory is O(N_T k).  There is no CPU
or eager path: a CPU tensor raises.  Nothing here is differentiable."""
import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .losses import _DTYPES, _features
from .pooling import check_ptr, ptr_on

MAX_K = 8
MAX_PARTS = 1024


def match_descriptors(xS, xT, k=1, ptr_S=None, ptr_T=None, exclude=None, parts=0):
    """(idx, d2): for every row a of xT the k rows b of xS with the smallest d2(a,b) = |xT[a] - xS[b]|^2, ordered by the pair
    (d2, b) ascending, so an exact tie goes to the lower row.  idx (N_T,k) int64 rows of xS, d2 (N_T,k) in the features' dtype,
    the bits of pair_sqdist; 1 <= k <= 8.  A NaN distance is never a match; a slot without a candidate (fewer than k rows to
    search, an excluded row, NaN) holds idx = -1 and d2 = +inf.
    ptr_S, ptr_T: both None, or the (B+1,) int64 range tables of two mini-batches of B meshes each (MeshBatch.ptr): the rows
    ptr_T[m]:ptr_T[m+1] of xT search the rows ptr_S[m]:ptr_S[m+1] of xS only; idx stays a row number of the whole xS.
    exclude: None, or (N_T,) int64 on the features' device: the one row of xS that row a skips (-1: none).
    parts: how many workgroups share the xS range of each 64-row tile of xT (0: the library chooses); the result does not
    depend on it.  Inputs are detached; views are made contiguous.  Without ptr tables nothing synchronises with the host
    (the call can be captured in a StepGraph); the tables' values are checked on the host as fieldconv_amd.pooling does."""
    what = 'match_descriptors'
    k = _whole(k, 1, MAX_K, what, 'k')
    parts = _whole(parts, 0, MAX_PARTS, what, 'parts')
    for name, x in (('xS', xS), ('xT', xT)):
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in _DTYPES:
            raise ValueError(f'{what}: {name} must be an (N,C) float32 or float64 tensor')
    if xS.dtype != xT.dtype or xS.shape[1] != xT.shape[1]:
        raise ValueError(f'{what}: xS {tuple(xS.shape)} {xS.dtype} and xT {tuple(xT.shape)} {xT.dtype} must share dtype and channel count')
    n_S, n_T, C = int(xS.shape[0]), int(xT.shape[0]), int(xS.shape[1])
    if (ptr_S is None) != (ptr_T is None):
        raise ValueError(f'{what}: ptr_S and ptr_T go together (the meshes of two mini-batches): give both or neither')
    if exclude is not None and (not torch.is_tensor(exclude) or exclude.dtype != torch.int64 or tuple(exclude.shape) != (n_T,)):
        raise ValueError(f'{what}: exclude must be a ({n_T},) int64 tensor (one row of xS per row of xT, -1: none), got '
                         f'{(tuple(exclude.shape), exclude.dtype) if torch.is_tensor(exclude) else type(exclude).__name__}')
    _features(xS, xT, what)
    dev, dt = xS.device, xS.dtype
    if exclude is not None:
        if exclude.device != dev:
            raise RuntimeError(f'{what}: exclude is on {exclude.device}, the features on {dev}')
        exclude = exclude.contiguous()
    B = 0
    if ptr_T is not None:
        host_T, host_S = check_ptr(ptr_T, n_T, what, 'ptr_T'), check_ptr(ptr_S, n_S, what, 'ptr_S')
        if len(host_T) != len(host_S):
            raise ValueError(f'{what}: ptr_T describes {len(host_T) - 1} meshes, ptr_S {len(host_S) - 1}')
        B = len(host_T) - 1
        if n_T + 64 * B >= 2 ** 31 - 1:
            raise ValueError(f'{what}: rows + 64 * meshes must stay below 2^31')
        ptr_T, ptr_S = ptr_on(ptr_T, host_T, dev), ptr_on(ptr_S, host_S, dev)
    lib = _lib.load()
    xSc, xTc = _by_value(xS.detach()), _by_value(xT.detach())
    with _on(dev):
        nbytes = lib.fc_match_workspace_bytes(n_T, k, parts)
        ws = _scratch(nbytes, dev, None)
        idx = torch.empty((n_T, k), dtype=torch.int64, device=dev)
        d2 = torch.empty((n_T, k), dtype=dt, device=dev)
        _lib.check(lib.fc_match_topk(_ptr(xSc), n_S, _ptr(xTc), n_T, C, _DTYPES[dt], _ptr(ptr_S), _ptr(ptr_T), B, _ptr(exclude), k, parts,
                                     _ptr(idx), _ptr(d2), _ptr(ws), nbytes, _stream()), 'fc_match_topk')
    return idx, d2


def mutual_matches(xS, xT, ptr_S=None, ptr_T=None):
    """(M,2) int64 rows [row of xT, row of xS], ascending by the first column: the pairs (a,b) where b is the nearest row of a
    and a is the nearest row of b (nearest by (d2, row), as match_descriptors orders them; the distance has the same bits in
    both directions).  Two kernel calls and plain torch; the number of rows is read back (one synchronisation)."""
    to_S, _ = match_descriptors(xS, xT, 1, ptr_S, ptr_T)
    to_T, _ = match_descriptors(xT, xS, 1, ptr_T, ptr_S)
    a = torch.arange(xT.shape[0], device=xT.device)
    b = to_S[:, 0]
    keep = (b >= 0) & (to_T[b.clamp(min=0), 0] == a)
    return torch.stack((a[keep], b[keep]), 1)


def match_accuracy(idx, pos_pairs):
    """(k,) float64 tensor: entry j is the share of the distinct xT rows listed in pos_pairs (P,2) whose true row of xS is among
    their first j + 1 matches idx[a, :j + 1] (idx (N_T,k) of match_descriptors).  Plain torch on the tensors' device."""
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int64 or idx.shape[1] < 1:
        raise ValueError('match_accuracy: idx must be an (N_T,k) int64 tensor')
    if not torch.is_tensor(pos_pairs) or pos_pairs.dim() != 2 or pos_pairs.shape[1] != 2 or pos_pairs.dtype != torch.int64:
        raise ValueError('match_accuracy: pos_pairs must be a (P,2) int64 tensor of [row of xT, row of xS]')
    if pos_pairs.device != idx.device:
        raise RuntimeError(f'match_accuracy: pos_pairs is on {pos_pairs.device}, idx on {idx.device}')
    if pos_pairs.shape[0] < 1:
        raise ValueError('match_accuracy: pos_pairs holds no pair')
    rows, of_row = torch.unique(pos_pairs[:, 0], return_inverse=True)
    found = (idx[pos_pairs[:, 0]] == pos_pairs[:, 1:2]).cumsum(1) > 0          # (P,k): pair p is matched within the first j + 1
    per_row = torch.zeros((rows.numel(), idx.shape[1]), dtype=torch.int64, device=idx.device).index_add_(0, of_row, found.to(torch.int64))
    hits = (per_row > 0).sum(0).to(torch.float64)
    # integer counts and one rounded division each (by a tensor: dividing by a Python number multiplies by its reciprocal on the device)
    return hits / torch.full_like(hits, rows.numel())
