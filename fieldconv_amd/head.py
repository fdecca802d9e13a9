"""The vertex-classification head on the device (csrc/fc_linear_ce.hip): a linear layer fused with cross-entropy, and with the
arg-max / top-k prediction.

The reference's correspondence network ends in `lin2 = Linear(256, n_classes)` + `CrossEntropyLoss` with n_classes = the number
of vertices, so the stock composite builds an N x K logit matrix four times over per step.  Here the logits never exist: every
kernel recomputes the 64 x 64 tile it needs with one routine, so memory is O(N H + K H + N parts) (plus O(K H parts) partial sums
of the weight gradient) and a logit has the same bits in the loss, in the gradients and in `linear_topk`.
float32 only, contiguous tensors only; there is no CPU or eager path: a CPU tensor raises."""
import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .matching import MAX_K

MAX_PARTS = 64
REDUCTIONS = ('none', 'mean', 'sum')


def _head_inputs(h, weight, bias, what, smoothed=False):
    """(N, H, K) of checked operands"""
    ops = (('h', h, 2, '(N,H)'), ('weight', weight, 2, '(K,H)')) + ((('bias', bias, 1, '(K,)'),) if bias is not None else ())
    for name, x, dim, shape in ops:
        if not torch.is_tensor(x) or x.dim() != dim:
            raise ValueError(f'{what}: {name} must be a {shape} tensor')
        if x.dtype != torch.float32:
            raise TypeError(f'{what}: {name} is {x.dtype}; the fused head is float32 only (float64 is not implemented)')
    N, H, K = int(h.shape[0]), int(h.shape[1]), int(weight.shape[0])
    if weight.shape[1] != H:
        raise ValueError(f'{what}: h {tuple(h.shape)} and weight {tuple(weight.shape)} must share their second dimension')
    if bias is not None and bias.shape[0] != K:
        raise ValueError(f'{what}: bias {tuple(bias.shape)} does not match weight {tuple(weight.shape)}')
    if N < 1 or H < 1 or K < 1:
        raise ValueError(f'{what}: empty operand (N, H, K) = {(N, H, K)}')
    if smoothed and K < 2:
        raise ValueError(f'{what}: smoothing > 0 needs at least two classes')
    for name, x, dim, shape in ops:
        if not x.is_contiguous():
            raise ValueError(f'{what}: {name} is not contiguous (call .contiguous() on it: the head copies nothing)')
        if x.is_neg():          # (float32 operands: no conjugate bit; memory under a lazy negative holds the opposite numbers)
            raise ValueError(f'{what}: {name} is a lazy negative (call .resolve_neg() on it: the head copies nothing)')
    for name, x, dim, shape in ops:
        if not x.is_cuda:
            raise RuntimeError(f'{what}: {name} is on {x.device}; the fused head runs on a ROCm device and has no CPU path')
        if x.device != h.device:
            raise RuntimeError(f'{what}: {name} is on {x.device}, h on {h.device}')
    if N >= 2 ** 30 or K >= 2 ** 30 or H > 2 ** 20 or N * H >= 2 ** 40 or K * H >= 2 ** 40:
        raise ValueError(f'{what}: (N, H, K) = {(N, H, K)} is beyond the kernels\' limits (N, K < 2^30, H <= 2^20)')
    return N, H, K


def _target(target, N, dev, what):
    if not torch.is_tensor(target) or target.dtype != torch.int64 or tuple(target.shape) != (N,):
        raise ValueError(f'{what}: target must be a ({N},) int64 tensor')
    if target.device != dev:
        raise RuntimeError(f'{what}: target is on {target.device}, h on {dev}')
    return target.contiguous()


def _forward(h, weight, bias, target, conf, off, ignore_index, parts):
    """(lse (N), loss_rows (N), total (3): sum, mean, counted rows) of detached, checked operands"""
    lib = _lib.load()
    N, H, K = int(h.shape[0]), int(h.shape[1]), int(weight.shape[0])
    dev = h.device
    with _on(dev):
        nbytes = lib.fc_linear_ce_workspace_bytes(N, H, K, parts, 0, 0)
        ws = _scratch(nbytes, dev, None)
        lse = torch.empty(N, dtype=torch.float32, device=dev)
        rows = torch.empty(N, dtype=torch.float32, device=dev)
        total = torch.empty(3, dtype=torch.float32, device=dev)
        _lib.check(lib.fc_linear_ce_forward(_ptr(h), _ptr(weight), _ptr(bias), _ptr(target), N, H, K, conf, off, ignore_index, parts,
                                            _ptr(lse), _ptr(rows), _ptr(total), _ptr(ws), nbytes, _stream()), 'fc_linear_ce_forward')
    return lse, rows, total


class _LinearCrossEntropy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, weight, bias, target, reduction, conf, off, ignore_index, parts):
        hd, wd, bd = h.detach(), weight.detach(), None if bias is None else bias.detach()
        lse, rows, total = _forward(hd, wd, bd, target, conf, off, ignore_index, parts)
        ctx.save_for_backward(hd, wd, bd, target, lse, total)
        ctx.head = (reduction, conf, off, ignore_index, parts)
        return rows if reduction == 'none' else total[0 if reduction == 'sum' else 1].view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        h, weight, bias, target, lse, total = ctx.saved_tensors
        reduction, conf, off, ignore_index, parts = ctx.head
        need_h, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2]
        N, H, K = int(h.shape[0]), int(h.shape[1]), int(weight.shape[0])
        dev = h.device
        g_h = g_w = g_b = None
        with _on(dev):
            g = g.detach().to(torch.float32)
            if reduction == 'none':
                scale = _by_value(g)
            else:          # the per-row upstream scale: g, or g / (rows that count)
                scale = _by_value((g if reduction == 'sum' else g / total[2]).reshape(1).expand(N))
            if need_h:
                g_h = torch.empty((N, H), dtype=torch.float32, device=dev)
                _lib.check(lib.fc_linear_ce_backward_input(_ptr(h), _ptr(weight), _ptr(bias), _ptr(target), _ptr(lse), _ptr(scale), N, H, K,
                                                           conf, off, ignore_index, _ptr(g_h), _stream()), 'fc_linear_ce_backward_input')
            if need_w or need_b:
                nbytes = lib.fc_linear_ce_workspace_bytes(N, H, K, parts, 1, 0)
                ws = _scratch(nbytes, dev, None)
                g_w = torch.empty((K, H), dtype=torch.float32, device=dev) if need_w else None
                g_b = torch.empty(K, dtype=torch.float32, device=dev) if need_b else None
                _lib.check(lib.fc_linear_ce_backward_weight(_ptr(h), _ptr(weight), _ptr(bias), _ptr(target), _ptr(lse), _ptr(scale), N, H, K,
                                                            conf, off, ignore_index, parts, _ptr(g_w), _ptr(g_b), _ptr(ws), nbytes,
                                                            _stream()), 'fc_linear_ce_backward_weight')
        return g_h, g_w, g_b, None, None, None, None, None, None


def linear_cross_entropy(h, weight, bias, target, reduction='mean', smoothing=0.0, ignore_index=-100, parts=0):
    """cross_entropy(h @ weight.T + bias, target) without the logits: h (N,H), weight (K,H), bias (K,) or None (a
    torch.nn.Linear), target (N,) int64.  reduction 'none' returns the (N,) per-row losses, 'sum' / 'mean' a scalar as
    torch.nn.functional.cross_entropy: rows whose target is ignore_index contribute 0 and do not count in the mean (all ignored:
    NaN).  Any other target outside [0,K) makes that row's loss (and every gradient it feeds) NaN; nothing is read for it.
    smoothing s: the true class weighs 1 - s, every other class s / (K - 1) (this package's LabelSmoothingLoss, the reference's).
    Gradients flow to h, weight and bias -- only to those that require one; the products of the others are not launched.
    parts: how many workgroups share the classes of a 64-row tile (and, in the weight gradient, the rows of a 64-class tile);
    0: the library chooses.  It changes the order of the sums -- the last bits -- only; two runs with the same parts give the
    same bits.  No host synchronisation."""
    what = 'linear_cross_entropy'
    if reduction not in REDUCTIONS:
        raise ValueError(f'{what}: reduction must be one of {REDUCTIONS}, got {reduction!r}')
    parts = _whole(parts, 0, MAX_PARTS, what, 'parts')
    ignore_index = _whole(ignore_index, -2 ** 63, 2 ** 63 - 1, what, 'ignore_index')
    s = float(smoothing)
    if not 0 <= s < 1:
        raise ValueError(f'{what}: smoothing must lie in [0, 1), got {smoothing!r}')
    N, H, K = _head_inputs(h, weight, bias, what, smoothed=s > 0)
    conf, off = 1.0 - s, (s / (K - 1) if s > 0 else 0.0)
    target = _target(target, N, h.device, what)
    return _LinearCrossEntropy.apply(h, weight, bias, target, reduction, conf, off, ignore_index, parts)


def linear_logsumexp(h, weight, bias, parts=0):
    """(N,) logsumexp of the rows of h @ weight.T + bias as the loss sees it (max first, the parts merged in order); not
    differentiable.  lse[n] >= every logit of row n that linear_topk returns."""
    what = 'linear_logsumexp'
    parts = _whole(parts, 0, MAX_PARTS, what, 'parts')
    N, H, K = _head_inputs(h, weight, bias, what)
    target = torch.full((N,), -100, dtype=torch.int64, device=h.device)
    return _forward(h.detach(), weight.detach(), None if bias is None else bias.detach(), target, 1.0, 0.0, -100, parts)[0]


def linear_topk(h, weight, bias, k=1, parts=0):
    """(idx, z): per row of h the k <= 8 classes with the largest logits of h @ weight.T + bias, ordered by (logit descending,
    class ascending): an exact tie goes to the lower class.  idx (N,k) int64, z (N,k) their logits -- bit for bit the ones
    linear_cross_entropy sees.  A NaN logit sorts after every number; slots beyond K hold idx = -1, z = -inf.  The order is total,
    so the result does not depend on parts.  Not differentiable; no host synchronisation."""
    what = 'linear_topk'
    k = _whole(k, 1, MAX_K, what, 'k')
    parts = _whole(parts, 0, MAX_PARTS, what, 'parts')
    N, H, K = _head_inputs(h, weight, bias, what)
    lib = _lib.load()
    dev = h.device
    hd, wd, bd = h.detach(), weight.detach(), None if bias is None else bias.detach()
    with _on(dev):
        nbytes = lib.fc_linear_ce_workspace_bytes(N, H, K, parts, 2, k)
        ws = _scratch(nbytes, dev, None)
        idx = torch.empty((N, k), dtype=torch.int64, device=dev)
        z = torch.empty((N, k), dtype=torch.float32, device=dev)
        _lib.check(lib.fc_linear_topk(_ptr(hd), _ptr(wd), _ptr(bd), N, H, K, k, parts, _ptr(idx), _ptr(z), _ptr(ws), nbytes, _stream()),
                   'fc_linear_topk')
    return idx, z


def vertex_accuracy(idx, target, ignore_index=-100):
    """(k,) float64 tensor: entry j is the share of the rows whose target (N,) int64 is among their first j + 1 predicted classes
    idx[n, :j + 1] (idx (N,k) of linear_topk); rows whose target is ignore_index (or negative) do not count.  Plain torch on the tensors' device."""
    if not torch.is_tensor(idx) or idx.dim() != 2 or idx.dtype != torch.int64 or idx.shape[1] < 1:
        raise ValueError('vertex_accuracy: idx must be an (N,k) int64 tensor')
    if not torch.is_tensor(target) or target.dtype != torch.int64 or tuple(target.shape) != (idx.shape[0],):
        raise ValueError(f'vertex_accuracy: target must be a ({idx.shape[0]},) int64 tensor')
    if target.device != idx.device:
        raise RuntimeError(f'vertex_accuracy: target is on {target.device}, idx on {idx.device}')
    counted = (target != ignore_index) & (target >= 0)
    found = ((idx == target[:, None]) & counted[:, None]).cumsum(1) > 0
    hits = found.sum(0).to(torch.float64)
    return hits / counted.sum().to(torch.float64)          # integer counts and one rounded division each; no synchronisation
