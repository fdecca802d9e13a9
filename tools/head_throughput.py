#!/usr/bin/env python3
"""The fused classification head against the stock composite on the same device (not part of bench.py).

The composite is F.cross_entropy(F.linear(h, W, b), target): it builds the N x K logits (100 MB at 4 999 x 4 999 in float32),
their log-softmax and their gradient.  linear_cross_entropy (csrc/fc_linear_ce.hip) recomputes logit tiles instead and keeps
O(N H + K H + N parts) memory.  This tool says what that costs or buys in time -- forward + backward with gradients to h, W and
b -- and in peak allocation, at

    (N, H, K) = (4 999, 256, 4 999),  (39 992, 256, 4 999),  (4 999, 256, 64)

and what the split over `parts` workgroups buys (parts = 1 against parts = 0).  Random float32 inputs, the same tensors for every
variant.  Device events around each repetition, the variants alternating inside one process after a common warm-up; medians
over --reps repetitions.  Writes one JSON object (--out) and prints it.

    python tools/head_throughput.py --out profiles/head_throughput.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(4999, 256, 4999), (39992, 256, 4999), (4999, 256, 64)]


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def compare(variants, warmup, reps):
    """{name: [ms, ...]} with the variants alternating"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, *ev))
    return out


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def peak_growth(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    del out
    return int(grown)


def case(N, H, K, args, dev):
    from fieldconv_amd.functional import linear_cross_entropy
    g = torch.Generator().manual_seed(N + K)
    h = torch.randn(N, H, generator=g).to(dev).requires_grad_(True)
    W = (torch.randn(K, H, generator=g) / H ** 0.5).to(dev).requires_grad_(True)
    b = torch.randn(K, generator=g).to(dev).requires_grad_(True)
    target = torch.randint(0, K, (N,), generator=g).to(dev)

    def step(loss_fn):
        return torch.autograd.grad(loss_fn(), [h, W, b])

    def fused(parts):
        return lambda: step(lambda: linear_cross_entropy(h, W, b, target, parts=parts))

    def dense():
        return step(lambda: torch.nn.functional.cross_entropy(torch.nn.functional.linear(h, W, b), target))

    variants = {'fused': fused(0), 'composite': dense, 'fused_parts_1': fused(1)}
    ms = compare(variants, args.warmup, args.reps)
    res = {name: summary(v) for name, v in ms.items()}
    ours, theirs = fused(0)(), dense()
    res.update(N=N, H=H, K=K,
               fused_over_composite=round(res['fused']['median_ms'] / res['composite']['median_ms'], 4),
               parts_0_over_parts_1=round(res['fused']['median_ms'] / res['fused_parts_1']['median_ms'], 4),
               peak_bytes_fused=peak_growth(fused(0)), peak_bytes_composite=peak_growth(dense),
               logits_bytes=4 * N * K,
               max_abs_difference={n: float((a - c).abs().max()) for n, a, c in zip(('g_h', 'g_W', 'g_b'), ours, theirs)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('head_throughput.py measures on a ROCm device and none is visible')
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), dtype='float32', what='forward + backward, gradients to h, W and b',
               cases=[case(*size, args, dev) for size in SIZES])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
