"""The reference's losses on the device (csrc/fc_loss.hip): functional forms and autograd functions under
fieldconv_amd.nn.TwinLoss, TwinEval and LabelSmoothingLoss.

Features are real (N,C) float32 or float64 tensors on a ROCm device; pair lists are (K,2) int64 rows [row of xT, row of xS].
There is no CPU or eager path: a CPU tensor raises.  Nothing here synchronises with the host except where a Python number is
returned (`pair_sqdist`'s index check, `twin_eval`, `twin_count_dense`)."""
import ctypes

import torch

from . import _lib
from ._launch import by_value as _by_value, on as _on, ptr as _ptr, scratch as _scratch, stream as _stream

_DTYPES = {torch.float32: 0, torch.float64: 1}
MAX_THRESHOLDS = 16


def _features(xS, xT, what):
    for name, x in (('xS', xS), ('xT', xT)):
        if not torch.is_tensor(x) or x.dim() != 2 or x.dtype not in _DTYPES:
            raise ValueError(f'{what}: {name} must be an (N,C) float32 or float64 tensor')
        if not x.is_cuda:
            raise RuntimeError(f'{what}: {name} is on {x.device}; fieldconv_amd losses run on a ROCm device and have no CPU path')
    if xS.dtype != xT.dtype or xS.device != xT.device or xS.shape[1] != xT.shape[1]:
        raise ValueError(f'{what}: xS {tuple(xS.shape)} {xS.dtype} {xS.device} and xT {tuple(xT.shape)} {xT.dtype} {xT.device} '
                         'must share dtype, device and channel count')
    if xS.shape[0] < 1 or xT.shape[0] < 1 or xS.shape[1] < 1:
        raise ValueError(f'{what}: empty features')
    if max(xS.shape[0], xT.shape[0]) >= 2 ** 24 or max(xS.shape[0], xT.shape[0]) * xS.shape[1] * 8 >= 2 ** 32:
        raise ValueError(f'{what}: rows beyond the 32-bit row limit (N < 2^24, N*C*8 < 4 GiB)')


def _pairs(pairs, dev, what, name):
    if not torch.is_tensor(pairs) or pairs.dim() != 2 or pairs.shape[1] != 2 or pairs.dtype != torch.int64:
        raise ValueError(f'{what}: {name} must be a (K,2) int64 tensor of [row of xT, row of xS]')
    if pairs.device != dev:
        raise RuntimeError(f'{what}: {name} is on {pairs.device}, the features on {dev}')
    return pairs.contiguous()


def _bad_pairs(pairs, n_T, n_S):
    """device bool: some index of the pair list lies outside [0,n_T) x [0,n_S)"""
    if pairs.shape[0] == 0:
        return torch.zeros((), dtype=torch.bool, device=pairs.device)
    lo = pairs.amin(0)
    hi = pairs.amax(0)
    return (lo[0] < 0) | (lo[1] < 0) | (hi[0] >= n_T) | (hi[1] >= n_S)


def _sqdist_unchecked(xS, xT, pairs):
    lib = _lib.load()
    K = int(pairs.shape[0])
    d2 = torch.empty(K, dtype=xS.dtype, device=xS.device)
    with _on(xS.device):
        _lib.check(lib.fc_pair_sqdist(_ptr(xS), xS.shape[0], _ptr(xT), xT.shape[0], xS.shape[1], _DTYPES[xS.dtype], _ptr(pairs), K,
                                      _ptr(d2), _stream()), 'fc_pair_sqdist')
    return d2


def pair_sqdist(xS, xT, pairs):
    """d2[k] = |xT[pairs[k,0]] - xS[pairs[k,1]]|^2, summed over the channels in ascending order with every operation rounded
    on its own (numpy in the same dtype restates it bit for bit).  Not differentiable.  An index outside the features raises
    IndexError (checked before the launch: one synchronisation)."""
    _features(xS, xT, 'pair_sqdist')
    pairs = _pairs(pairs, xS.device, 'pair_sqdist', 'pairs')
    if bool(_bad_pairs(pairs, xT.shape[0], xS.shape[0])):
        raise IndexError(f'pair_sqdist: pair index outside xT ({xT.shape[0]} rows) x xS ({xS.shape[0]} rows)')
    return _sqdist_unchecked(_by_value(xS.detach()), _by_value(xT.detach()), pairs)


def _row_segments(rows, n):
    """(rowptr (n+1), order (K)): the positions of `rows` sorted stably by value, and each value's range in that order."""
    srt, order = torch.sort(rows, stable=True)
    rowptr = torch.searchsorted(srt, torch.arange(n + 1, device=rows.device, dtype=rows.dtype))
    return rowptr, order


class _TwinLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xS, xT, p_, n_, yN, mu):
        lib = _lib.load()
        xSc, xTc = _by_value(xS.detach()), _by_value(xT.detach())
        P, M = int(p_.shape[0]), int(n_.shape[0])
        dev, dt = xS.device, xS.dtype
        with _on(dev):
            nbytes = lib.fc_twin_loss_workspace_bytes(P, M)
            ws = _scratch(nbytes, dev)
            d2 = torch.empty(P + M, dtype=dt, device=dev)
            loss = torch.empty(1, dtype=dt, device=dev)
            _lib.check(lib.fc_twin_loss_forward(_ptr(xSc), xSc.shape[0], _ptr(xTc), xTc.shape[0], xSc.shape[1], _DTYPES[dt], _ptr(p_), P,
                                                _ptr(n_), M, _ptr(yN), float(mu), _ptr(d2), _ptr(loss), _ptr(ws), nbytes, _stream()),
                       'fc_twin_loss_forward')
        ctx.save_for_backward(xSc, xTc, p_, n_, yN, d2)
        ctx.mu = float(mu)
        return loss

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        xS, xT, p_, n_, yN, d2 = ctx.saved_tensors
        P, M = int(p_.shape[0]), int(n_.shape[0])
        dev, dt = xS.device, xS.dtype
        with _on(dev):
            # the pairs at each row, in list order (torch's stable sort on the device; nothing comes back to the host)
            rows = torch.cat((p_, n_), 0)
            rowptr_T, order_T = _row_segments(rows[:, 0].contiguous(), xT.shape[0])
            rowptr_S, order_S = _row_segments(rows[:, 1].contiguous(), xS.shape[0])
            g = _by_value(g.detach().to(dt))
            gT = torch.empty(tuple(xT.shape), dtype=dt, device=dev)
            gS = torch.empty(tuple(xS.shape), dtype=dt, device=dev)
            _lib.check(lib.fc_twin_loss_backward(_ptr(xS), xS.shape[0], _ptr(xT), xT.shape[0], xS.shape[1], _DTYPES[dt], _ptr(p_), P,
                                                 _ptr(n_), M, _ptr(yN), ctx.mu, _ptr(d2), _ptr(g), _ptr(rowptr_T), _ptr(order_T),
                                                 _ptr(rowptr_S), _ptr(order_S), _ptr(gT), _ptr(gS), _stream()), 'fc_twin_loss_backward')
        return gS, gT, None, None, None, None


def twin_loss(xS, xT, p_, n_, yN, mu=5):
    """(1,) tensor in the features' dtype:
        sum_k d2(p_k) / P + sum_k [ yN_k d2(n_k) + (1 - yN_k) max(mu - d2(n_k), 0) ] / M
    (the reference's TwinLoss with its random weights yN (M) passed in; they are used as float32, and 1 - yN is rounded in float32
    whatever the features' dtype, as in the reference).  Gradients flow to xS and xT; both are dense (N,C),
    each row the sum of its pairs' contributions in list order, the same bits on every run.  No host synchronisation: the
    indices are not checked here, and a pair outside the features makes the loss NaN."""
    _features(xS, xT, 'twin_loss')
    dev = xS.device
    p_ = _pairs(p_, dev, 'twin_loss', 'p_')
    n_ = _pairs(n_, dev, 'twin_loss', 'n_')
    if p_.shape[0] < 1 or n_.shape[0] < 1:
        raise ValueError('twin_loss: p_ and n_ must each hold at least one pair')
    if not torch.is_tensor(yN) or yN.shape != (n_.shape[0],) or yN.device != dev or not yN.is_floating_point():
        raise ValueError(f'twin_loss: yN must be a ({n_.shape[0]},) floating-point tensor on {dev}')
    return _TwinLoss.apply(xS, xT, p_, n_, _by_value(yN.detach().to(torch.float32)), float(mu))


def twin_count_dense(xS, xT, thresholds):
    """(below, above): int64 device tensors (T,), below[t] = #{(a,b) in [0,N_T) x [0,N_S) : d2(a,b) < thresholds[t]} and above[t] the
    same with >, for up to 16 thresholds (Python numbers, rounded to the features' dtype) in one pass over all N_T*N_S pairs; no
    pair list exists at any point.  d2 as in pair_sqdist, bit for bit."""
    _features(xS, xT, 'twin_count_dense')
    thr = [float(t) for t in thresholds]
    if not 1 <= len(thr) <= MAX_THRESHOLDS:
        raise ValueError(f'twin_count_dense: between 1 and {MAX_THRESHOLDS} thresholds, got {len(thr)}')
    lib = _lib.load()
    xSc, xTc = _by_value(xS.detach()), _by_value(xT.detach())
    T = len(thr)
    with _on(xS.device):
        counts = torch.empty(2 * T, dtype=torch.int64, device=xS.device)
        _lib.check(lib.fc_twin_count_dense(_ptr(xSc), xSc.shape[0], _ptr(xTc), xTc.shape[0], xSc.shape[1], _DTYPES[xS.dtype],
                                           (ctypes.c_double * T)(*thr), T, _ptr(counts), _stream()), 'fc_twin_count_dense')
    return counts[:T], counts[T:]


def twin_eval(xS, xT, p_, n_, thresh):
    """(nFN, nFP) Python ints: #{d2(p_k) > thresh} and #{d2(n_k) < thresh} (the reference's TwinEval).  n_ = None: every pair
    of [0,N_T) x [0,N_S) that is not in p_ -- counted densely, minus the distinct pairs of p_ (the same d2 bits, so the
    difference is exact).  One synchronisation, at the end; an index outside the features raises IndexError."""
    _features(xS, xT, 'twin_eval')
    dev = xS.device
    n_T, n_S = int(xT.shape[0]), int(xS.shape[0])
    p_ = _pairs(p_, dev, 'twin_eval', 'p_')
    xSc, xTc = _by_value(xS.detach()), _by_value(xT.detach())
    thr = torch.tensor(float(thresh), dtype=xS.dtype).item()          # the threshold as the features' dtype holds it
    limit = torch.tensor([n_T - 1, n_S - 1], device=dev)
    zero = torch.zeros(2, dtype=torch.int64, device=dev)
    bad = _bad_pairs(p_, n_T, n_S)
    dp = _sqdist_unchecked(xSc, xTc, torch.minimum(torch.maximum(p_, zero), limit))
    n_fn = (dp > thr).sum()
    if n_ is None:
        below, _ = twin_count_dense(xSc, xTc, [thr])
        lin = torch.unique(p_[:, 0] * n_S + p_[:, 1])
        distinct = torch.stack((torch.div(lin, n_S, rounding_mode='floor'), lin % n_S), 1)
        dd = _sqdist_unchecked(xSc, xTc, torch.minimum(torch.maximum(distinct, zero), limit))
        n_fp = below[0] - (dd < thr).sum()
    else:
        n_ = _pairs(n_, dev, 'twin_eval', 'n_')
        bad = bad | _bad_pairs(n_, n_T, n_S)
        dn = _sqdist_unchecked(xSc, xTc, torch.minimum(torch.maximum(n_, zero), limit))
        n_fp = (dn < thr).sum()
    out = torch.stack((n_fn, n_fp, bad.to(torch.int64))).tolist()          # the one synchronisation
    if out[2]:
        raise IndexError(f'twin_eval: pair index outside xT ({n_T} rows) x xS ({n_S} rows)')
    return out[0], out[1]


class _LabelSmoothing(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, weight, conf, off):
        lib = _lib.load()
        x = _by_value(pred.detach())
        weight = None if weight is None else _by_value(weight)
        N, K = int(x.shape[0]), int(x.shape[1])
        dev, dt = x.device, x.dtype
        with _on(dev):
            nbytes = lib.fc_label_smoothing_workspace_bytes(N, K)
            ws = _scratch(nbytes, dev)
            loss = torch.empty(1, dtype=dt, device=dev)
            _lib.check(lib.fc_label_smoothing_forward(_ptr(x), _ptr(target), _ptr(weight), N, K, _DTYPES[dt], conf, off, _ptr(loss),
                                                      _ptr(ws), nbytes, _stream()), 'fc_label_smoothing_forward')
        ctx.save_for_backward(x, target, weight)
        ctx.conf, ctx.off = conf, off
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        lib = _lib.load()
        x, target, weight = ctx.saved_tensors
        N, K = int(x.shape[0]), int(x.shape[1])
        with _on(x.device):
            g = _by_value(g.detach().to(x.dtype).reshape(1))
            gpred = torch.empty((N, K), dtype=x.dtype, device=x.device)
            _lib.check(lib.fc_label_smoothing_backward(_ptr(x), _ptr(target), _ptr(weight), _ptr(g), N, K, _DTYPES[x.dtype], ctx.conf,
                                                       ctx.off, _ptr(gpred), _stream()), 'fc_label_smoothing_backward')
        return gpred, None, None, None, None


def check_smoothing(classes, smoothing):
    if isinstance(classes, bool) or int(classes) != classes or classes < 2:
        raise ValueError(f'label smoothing: classes must be an integer >= 2, got {classes!r}')
    if not 0 <= smoothing < 1:
        raise ValueError(f'label smoothing: smoothing must lie in [0, 1), got {smoothing!r}')


def label_smoothing_loss(pred, target, classes, smoothing=0.0, weight=None):
    """Scalar mean_n sum_k -t_nk w_k log_softmax(pred_n)_k for pred (N,K) and target (N) int64, t_nk = 1 - smoothing at the
    target and smoothing / (classes - 1) elsewhere -- `classes` as given, which need not be K (the reference's
    LabelSmoothingLoss); weight (K) optional.  Gradient flows to pred only."""
    check_smoothing(classes, smoothing)
    if not torch.is_tensor(pred) or pred.dim() != 2 or pred.dtype not in _DTYPES:
        raise ValueError('label_smoothing_loss: pred must be an (N,K) float32 or float64 tensor')
    if not pred.is_cuda:
        raise RuntimeError(f'label_smoothing_loss: pred is on {pred.device}; fieldconv_amd losses run on a ROCm device and have no CPU path')
    N, K = pred.shape
    if N < 1 or K < 1:
        raise ValueError('label_smoothing_loss: empty pred')
    if not torch.is_tensor(target) or target.shape != (N,) or target.dtype != torch.int64 or target.device != pred.device:
        raise ValueError(f'label_smoothing_loss: target must be a ({N},) int64 tensor on {pred.device}')
    if weight is not None:
        if not torch.is_tensor(weight) or weight.shape != (K,) or weight.device != pred.device or not weight.is_floating_point():
            raise ValueError(f'label_smoothing_loss: weight must be a ({K},) floating-point tensor on {pred.device}')
        weight = weight.detach().to(pred.dtype)          # (taken by value in the node)
    return _LabelSmoothing.apply(pred, target.contiguous(), weight, 1.0 - float(smoothing), float(smoothing) / (int(classes) - 1))
