#!/usr/bin/env python3
"""match_descriptors against the dense way on the same device (not part of bench.py).

The dense way is torch.cdist(xT, xS).pow(2).topk(k, largest=False): it builds the N_T x N_S matrix (1.6 GB at 20 000 rows in
float32) and its distances are not the losses' bits; match_descriptors (csrc/fc_match.hip) keeps O(N_T k) memory, orders exact
ties by row and returns the bits of pair_sqdist.  This tool only says what that costs or buys in time, at

    (N_T, N_S, C) = (2 048, 2 048, 16) k = 1,  (4 999, 4 999, 32) k = 1,  (20 000, 20 000, 16) k = 8

and, at the first size, what the split of the xS range over several workgroups buys (parts = 1 against parts = 0: 32 tiles of
xT are 32 workgroups on 256 CUs without it).  Random float32 features, the same tensors for every variant.  Device events
around each repetition, the variants alternating inside one process after a common warm-up; medians over --reps repetitions.
Also recorded: the peak allocation growth of one call of each way, and how many rows the two ways match differently (the
dense distances are rounded differently, so near ties can swap).  Writes one JSON object (--out) and prints it.

    python tools/match_throughput.py --out profiles/match_throughput.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = [(2048, 2048, 16, 1), (4999, 4999, 32, 1), (20000, 20000, 16, 8)]


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


def case(n_T, n_S, C, k, args, dev, with_parts):
    from fieldconv_amd.functional import match_descriptors
    g = torch.Generator().manual_seed(n_T + C)
    xS, xT = torch.rand(n_S, C, generator=g).to(dev), torch.rand(n_T, C, generator=g).to(dev)

    def dense():
        return torch.cdist(xT, xS).pow(2).topk(k, dim=1, largest=False)

    variants = {'match_descriptors': lambda: match_descriptors(xS, xT, k=k), 'cdist_topk': dense}
    if with_parts:
        variants['match_descriptors_parts_1'] = lambda: match_descriptors(xS, xT, k=k, parts=1)
    ms = compare(variants, args.warmup, args.reps)
    res = {name: summary(v) for name, v in ms.items()}
    idx = match_descriptors(xS, xT, k=k)[0]
    res.update(N_T=n_T, N_S=n_S, C=C, k=k,
               match_over_cdist=round(res['match_descriptors']['median_ms'] / res['cdist_topk']['median_ms'], 4),
               peak_bytes_match=peak_growth(lambda: match_descriptors(xS, xT, k=k)), peak_bytes_cdist=peak_growth(dense),
               rows_matched_differently=int((idx != dense()[1]).any(1).sum()))
    if with_parts:
        res['parts_0_over_parts_1'] = round(res['match_descriptors']['median_ms'] / res['match_descriptors_parts_1']['median_ms'], 4)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('match_throughput.py measures on a ROCm device and none is visible')
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), dtype='float32',
               cases=[case(*size, args, dev, with_parts=(i == 0)) for i, size in enumerate(SIZES)])
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
