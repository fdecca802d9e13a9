"""Time the selection kernels themselves, every rung of their K ladders (match_throughput.py times one k per size and
head_throughput.py times the loss, not linear_topk): device events, `--warmup` calls, median of `--reps`.

  linear_topk        head_throughput.py's two large sizes, k = 1, 2, 4, 8, parts = 0 and 1
  match_descriptors  match_throughput.py's two large sizes, k = 1, 2, 4, 8, parts = 0 and 1
  knn_weights        100 000 rows of 5 to 40 candidates (the row lengths interpolation_plan produces), k = 3, 8, 16, power 2

    python tools/selection_ladder.py            # prints one JSON object {case: median ms}

A/B against another build of the library: FIELDCONV_HIP_LIB=/path/to/libfieldconv_hip.so (profiles/selection_ab.txt).
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return round(statistics.median(ms), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('selection_ladder.py measures on a ROCm device and none is visible')
    from fieldconv_amd.functional import knn_weights, linear_topk, match_descriptors
    dev = torch.device('cuda:0')
    out = {}
    for N, H, K in [(4999, 256, 4999), (39992, 256, 4999)]:
        g = torch.Generator().manual_seed(N + K)
        h, W, b = torch.randn(N, H, generator=g).to(dev), (torch.randn(K, H, generator=g) / H ** 0.5).to(dev), torch.randn(K, generator=g).to(dev)
        for k in (1, 2, 4, 8):
            for parts in (0, 1):
                out['linear_topk/N%d_K%d/k%d/parts%d' % (N, K, k, parts)] = median_ms(lambda: linear_topk(h, W, b, k, parts), args.warmup, args.reps)
    for n_T, n_S, C in [(4999, 4999, 32), (20000, 20000, 16)]:
        g = torch.Generator().manual_seed(n_T + C)
        xS, xT = torch.rand(n_S, C, generator=g).to(dev), torch.rand(n_T, C, generator=g).to(dev)
        for k in (1, 2, 4, 8):
            for parts in (0, 1):
                out['match_descriptors/T%d_S%d_C%d/k%d/parts%d' % (n_T, n_S, C, k, parts)] = median_ms(
                    lambda: match_descriptors(xS, xT, k=k, parts=parts), args.warmup, args.reps)
    g = torch.Generator().manual_seed(7)
    n_f = 100000
    lengths = torch.randint(5, 41, (n_f,), generator=g)
    rowptr = torch.zeros(n_f + 1, dtype=torch.int64)
    rowptr[1:] = lengths.cumsum(0)
    n_slots = int(rowptr[-1])
    cand = torch.randint(0, 2500, (n_slots,), generator=g).to(torch.int32).to(dev)
    dist = torch.rand(n_slots, generator=g).to(dev)
    rowptr = rowptr.to(torch.int32).to(dev)
    for k in (3, 8, 16):
        out['knn_weights/rows%d_slots%d/k%d' % (n_f, n_slots, k)] = median_ms(lambda: knn_weights(rowptr, cand, dist, k, 2), args.warmup, args.reps)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
