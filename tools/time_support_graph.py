#!/usr/bin/env python3
"""Time the support-graph kernels (farthest-point sampling, radius neighbours: fieldconv_amd.transforms) with HIP events,
against the numpy / scipy restatement of the same contract on the host of the same box.  Points: a jittered Fibonacci
sampling of the sphere of unit area (what NormalizeArea makes of a sphere mesh).  Prints a markdown table; also checks that
the device results equal the restatement's.

    python tools/time_support_graph.py [--reps R]
"""
import argparse
import math
import os
import sys
import time

import numpy as np
import torch
from scipy.spatial import cKDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fieldconv_amd.transforms import farthest_point_sample, radius_edges  # noqa: E402

# (label, points, samples, epsilon, max_num_neighbors)
CASES = [('FAUST size, all points', 6890, 6890, 0.2, 512),
         ('segmentation: 12 500 -> 1 024, eps 0.2', 12500, 1024, 0.2, 512),
         ('20 000 points', 20000, 1024, 0.05, 512),
         ('160 000 points', 160000, 1024, 0.02, 512)]


def unit_area_sphere(N, seed=0):
    i = np.arange(N, dtype=np.float64)
    z = 1.0 - 2.0 * (i + 0.5) / N
    rad = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    lon = math.pi * (3.0 - math.sqrt(5.0)) * i
    p = np.stack((rad * np.cos(lon), rad * np.sin(lon), z), 1)
    p = p + (0.15 / math.sqrt(N)) * np.random.default_rng(seed).standard_normal((N, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    return (p / math.sqrt(4 * math.pi)).astype(np.float32)


def sq_dist(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def fps_host(p, S, start):
    mind = np.full(p.shape[0], np.inf, dtype=np.float32)
    taken = np.zeros(p.shape[0], dtype=bool)
    out = np.empty(S, dtype=np.int64)
    last = start
    for k in range(S):
        out[k] = last
        taken[last] = True
        if k + 1 == S:
            break
        np.minimum(mind, sq_dist(p, p[last]), out=mind)
        last = int(np.argmax(np.where(taken, np.float32(-1), mind)))
    return out


def radius_host(p, eps, K):
    N = p.shape[0]
    r2 = np.float32(eps) * np.float32(eps)
    pairs = cKDTree(p.astype(np.float64)).query_pairs(float(np.sqrt(np.float64(r2))) * (1 + 1e-4) + 1e-7, output_type='ndarray')
    q = np.concatenate((pairs[:, 0], pairs[:, 1], np.arange(N)))
    n = np.concatenate((pairs[:, 1], pairs[:, 0], np.arange(N)))
    d2 = sq_dist(p[n], p[q])
    m = d2 < r2
    q, n, d2 = q[m], n[m], d2[m]
    order = np.lexsort((n, d2, q))
    q, n = q[order], n[order]
    keep = (np.arange(q.size) - np.searchsorted(q, q, side='left')) < K
    q, n = q[keep], n[keep]
    order = np.lexsort((n, q))
    return np.stack((q[order], n[order]), 1)


def device_ms(fn, reps):
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times)), out


def host_ms(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs a ROCm device'
    dev = torch.device('cuda:0')
    print('device: %s' % torch.cuda.get_device_name(dev))
    print('| case | N | S | eps | E | FPS device ms | FPS host ms | radius device ms | radius host ms | equal |')
    print('|---|---|---|---|---|---|---|---|---|---|')
    for label, N, S, eps, K in CASES:
        p = unit_area_sphere(N)
        pd = torch.from_numpy(p).to(dev)
        f_dev, idx = device_ms(lambda: farthest_point_sample(pd, S, 0), args.reps)
        f_host, idx_ref = host_ms(lambda: fps_host(p, S, 0))
        sub = np.sort(idx_ref)
        ps = np.ascontiguousarray(p[sub])
        psd = torch.from_numpy(ps).to(dev)
        r_dev, edges = device_ms(lambda: radius_edges(psd, eps, K), args.reps)     # (includes the one synchronisation on E)
        r_host, edges_ref = host_ms(lambda: radius_host(ps, eps, K))
        same = np.array_equal(idx.cpu().numpy(), idx_ref) and np.array_equal(edges.cpu().numpy(), edges_ref)
        print('| %s | %d | %d | %g | %d | %.3f | %.1f | %.3f | %.1f | %s |' % (label, N, S, eps, edges.shape[0], f_dev, f_host, r_dev,
                                                                          r_host, 'yes' if same else 'NO'), flush=True)
    # the radius search over every point at the two large sizes (the all-pairs scan's cost)
    for N, eps in ((20000, 0.05), (160000, 0.02)):
        p = unit_area_sphere(N)
        pd = torch.from_numpy(p).to(dev)
        r_dev, edges = device_ms(lambda: radius_edges(pd, eps, 512), args.reps)
        r_host, edges_ref = host_ms(lambda: radius_host(p, eps, 512))
        same = np.array_equal(edges.cpu().numpy(), edges_ref)
        print('| radius over all %d points | %d | - | %g | %d | - | - | %.3f | %.1f | %s |' % (N, N, eps, edges.shape[0], r_dev, r_host,
                                                                                     'yes' if same else 'NO'), flush=True)


if __name__ == '__main__':
    main()
