#!/usr/bin/env python3
"""Time the feature-matching head (fieldconv_amd.nn.TwinLoss / TwinEval, fieldconv_amd.utils pair utilities) and
LabelSmoothingLoss with HIP events (median of --reps after a warm-up), each against other code doing the same job: the
notebook's getNullPairs + randperm restated in numpy / torch on this box's CPU, and the same formulas in stock torch ops on
the same GPU.  Prints markdown tables; the dense count's rate is given in pair-channel operations (3 per pair and channel:
subtract, multiply, add).

    python tools/time_twin_head.py [--reps R]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fieldconv_amd.losses import label_smoothing_loss, twin_loss  # noqa: E402
from fieldconv_amd.utils import null_pair_count, null_pairs_from_rank, sample_null_pairs, twin_eval_curve  # noqa: E402


def device_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def wall_ms(fn, reps):
    fn()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def notebook_null_pairs(pos_pairs, n):
    """what the notebook's getNullPairs computes, on the CPU, followed by its randperm pick of 512"""
    pos_lin = pos_pairs[0] * n + pos_pairs[1]
    null_lin = torch.from_numpy(np.setdiff1d(np.arange(n * n), pos_lin.numpy())).long()
    b = torch.remainder(null_lin, n)
    pairs = torch.stack((torch.div(null_lin - b, n, rounding_mode='floor'), b), 1)
    return pairs[torch.randperm(pairs.size(0))[:512]]


def stock_twin(xS, xT, p_, n_, yN, mu):
    lP = torch.sum(torch.pow(xT[p_[:, 0], :] - xS[p_[:, 1], :], 2), (0, 1)) / p_.size(0)
    lN = torch.sum(torch.pow(xT[n_[:, 0], :] - xS[n_[:, 1], :], 2), dim=1)
    return lP + (torch.sum(lN * yN) + torch.sum(torch.relu(mu - lN) * (1 - yN))) / n_.size(0)


def stock_smoothing(pred, target, classes, smoothing):
    logp = pred.log_softmax(dim=1)
    with torch.no_grad():
        t = torch.zeros_like(logp)
        t.fill_(smoothing / (classes - 1))
        t.scatter_(1, target.unsqueeze(1), 1.0 - smoothing)
    return torch.mean(torch.sum(-t * logp, dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--only', default='', help='twin | smoothing: run one family once (for a kernel trace), no tables')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a ROCm device'
    dev = torch.device('cuda:0')
    C, P, M, mu = 16, 512, 512, 5.0
    if args.only:
        torch.manual_seed(0)
        N = 2048
        xS, xT = (0.9 * torch.rand(N, C, device=dev)).requires_grad_(True), (0.9 * torch.rand(N, C, device=dev)).requires_grad_(True)
        pos = torch.stack((torch.arange(N, device=dev), torch.randperm(N, device=dev)), 1)[:P].contiguous()
        neg = sample_null_pairs(pos, N, N, M)
        yN = 0.2 * torch.rand(M, device=dev)
        pred = torch.randn(1024, 8, device=dev, requires_grad=True)
        target = torch.randint(0, 8, (1024,), device=dev)
        fns = {'twin': lambda: torch.autograd.grad(twin_loss(xS, xT, pos, neg, yN, mu), [xS, xT]),
               'twin-stock': lambda: torch.autograd.grad(stock_twin(xS, xT, pos, neg, yN, mu), [xS, xT]),
               'smoothing': lambda: torch.autograd.grad(label_smoothing_loss(pred, target, 8, 0.2), [pred]),
               'smoothing-stock': lambda: torch.autograd.grad(stock_smoothing(pred, target, 8, 0.2), [pred])}
        fns[args.only]()
        torch.cuda.synchronize()
        return
    print('device: %s' % torch.cuda.get_device_name(dev))
    print('| N | step | this package | compared with | ms | ms (other) |')
    print('|---|---|---|---|---|---|')
    for N in (2048, 6890):
        torch.manual_seed(0)
        xS, xT = (0.9 * torch.rand(N, C, device=dev)).requires_grad_(True), (0.9 * torch.rand(N, C, device=dev)).requires_grad_(True)
        perm = torch.randperm(N)
        pos_all = torch.stack((torch.arange(N), perm), 1)
        pos_dev = pos_all.to(dev)
        t_ours = wall_ms(lambda: sample_null_pairs(pos_dev, N, N, M), args.reps)
        t0 = time.perf_counter()
        notebook_null_pairs(pos_all, N)
        t_nb = (time.perf_counter() - t0) * 1e3
        print('| %d | negatives for one step | sample_null_pairs (wall, device) | getNullPairs + randperm restated on the CPU (one run) | %.3f | %.1f |'
              % (N, t_ours, t_nb), flush=True)
        p_ = pos_dev[:P].contiguous()
        n_ = sample_null_pairs(pos_dev, N, N, M)
        yN = 0.2 * torch.rand(M, device=dev)
        t_ours = device_ms(lambda: torch.autograd.grad(twin_loss(xS, xT, p_, n_, yN, mu), [xS, xT]), args.reps)
        t_stock = device_ms(lambda: torch.autograd.grad(stock_twin(xS, xT, p_, n_, yN, mu), [xS, xT]), args.reps)
        print('| %d | TwinLoss forward + backward, P = M = 512 | twin_loss | stock torch ops, same GPU | %.3f | %.3f |' % (N, t_ours, t_stock), flush=True)
        xSd, xTd = xS.detach(), xT.detach()
        for n_thr in (1, 16):
            thr = [2.5] if n_thr == 1 else [0.25 * (k + 1) for k in range(16)]
            t_ours = device_ms(lambda: twin_eval_curve(xSd, xTd, pos_dev, thr), args.reps)
            from fieldconv_amd.losses import twin_count_dense
            t_kernel = device_ms(lambda: twin_count_dense(xSd, xTd, thr), args.reps)
            rate = 3.0 * N * N * C / (t_kernel * 1e-3) / 1e12
            other = '-'
            if N == 2048:
                count = null_pair_count(pos_dev, N, N)
                n_all = null_pairs_from_rank(pos_dev, N, N, torch.arange(count, device=dev))          # the materialised list (67 MB)

                def stock_eval():
                    dn = torch.sum(torch.pow(xTd[n_all[:, 0], :] - xSd[n_all[:, 1], :], 2), dim=1)
                    return [torch.nonzero(dn < t).size(0) for t in thr]
                other = '%.3f' % device_ms(stock_eval, args.reps)
                del n_all
            print('| %d | TwinEval over the whole complement, %d threshold(s) | twin_eval_curve (dense kernel alone: %.3f ms, %.2f T pair-channel '
                  'op/s) | stock torch through a materialised pair list, same GPU | %.3f | %s |' % (N, n_thr, t_kernel, rate, t_ours, other), flush=True)
    pred = torch.randn(1024, 8, device=dev, requires_grad=True)
    target = torch.randint(0, 8, (1024,), device=dev)
    t_ours = device_ms(lambda: torch.autograd.grad(label_smoothing_loss(pred, target, 8, 0.2), [pred]), args.reps)
    t_stock = device_ms(lambda: torch.autograd.grad(stock_smoothing(pred, target, 8, 0.2), [pred]), args.reps)
    print('| 1024 x 8 | LabelSmoothingLoss forward + backward | label_smoothing_loss | the reference\'s op sequence in stock torch, same GPU | %.3f | %.3f |'
          % (t_ours, t_stock), flush=True)


if __name__ == '__main__':
    main()
