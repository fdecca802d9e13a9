#!/usr/bin/env python3
"""Mesh geodesics on the device against scipy.sparse.csgraph.dijkstra on the same box and the same graph (not part of bench.py).

    rows        all 4 999 distance rows of a 4 999-vertex mesh (geodesic_distances; scipy: one call with every index)
    nearest     12 500 vertices -> 1 024 samples, nearest sample + weights (sample_weights; scipy: min_only Dijkstra with
                its sources, then np.add.at of float64 masses)
    batch       8 such meshes as one MeshBatch-style call against 8 single calls (both on the device)
    large       one 160 000-vertex mesh -> 1 024 samples: over the LDS capacity, the one-workgroup global-memory path

Meshes: random points of the unit square, Delaunay-triangulated and lifted by a smooth height; samples by the package's FPS.
The edge graph is built once per mesh and passed in (graph=): what is timed is the solve, its launches and its torch glue.
Device events around each repetition after a common warm-up, median of --reps (5); scipy by perf_counter, median of
--scipy-reps.  Sweep counts (distance loop, label loop) are recorded beside the times.  Writes one JSON object (--out).

    python tools/geodesic_throughput.py --out profiles/geodesic_throughput.json
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(n, seed):
    from scipy.spatial import Delaunay
    rng = np.random.default_rng(seed)
    xy = rng.random((n, 2))
    z = 0.3 * np.sin(3.0 * xy[:, 0]) * np.cos(2.0 * xy[:, 1])
    pos = np.concatenate((xy, z[:, None]), 1).astype(np.float32)
    return torch.from_numpy(pos), torch.from_numpy(np.ascontiguousarray(Delaunay(xy).simplices.T.astype(np.int64)))


def device_ms(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ms = []
    for _ in range(reps):
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        ms.append(start.elapsed_time(stop))
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=reps)


def host_ms(fn, reps):
    ms = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        ms.append(1e3 * (time.perf_counter() - t))
    return dict(median_ms=round(statistics.median(ms), 3), min_ms=round(min(ms), 3), max_ms=round(max(ms), 3), reps=reps)


def scipy_graph(graph, V):
    import scipy.sparse as sp
    ptr, nbr, length = (t.cpu().numpy() for t in graph)
    return sp.csr_matrix((length.astype(np.float64), nbr, ptr), shape=(V, V))


def mesh_on(n, seed, dev, n_samples=None):
    from fieldconv_amd.geodesic import mesh_edge_graph
    from fieldconv_amd.transforms import farthest_point_sample
    pos, face = surface(n, seed)
    pos, face = pos.to(dev), face.to(dev)
    samples = None if n_samples is None else farthest_point_sample(pos, n_samples, 0).sort()[0]
    return pos, face, mesh_edge_graph(pos, face), samples


def ratio(a, b):
    return round(a['median_ms'] / b['median_ms'], 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scipy-reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geodesic_throughput.py measures on a ROCm device and none is visible')
    from scipy.sparse.csgraph import dijkstra
    from fieldconv_amd import geodesic as G
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), lds_vertices=G.LDS_VERTICES, cases={})

    # ---- all rows of a 4 999-vertex template
    pos, face, graph, _ = mesh_on(4999, 1, dev)
    every = torch.arange(4999, device=dev)
    _, sweeps = G.geodesic_distances(pos, face, every, graph=graph, return_sweeps=True)
    ours = device_ms(lambda: G.geodesic_distances(pos, face, every, graph=graph), args.warmup, args.reps)
    sg = scipy_graph(graph, 4999)
    theirs = host_ms(lambda: dijkstra(sg, indices=np.arange(4999)), args.scipy_reps)
    res['cases']['rows_4999x4999'] = dict(device=ours, scipy=theirs, device_over_scipy=ratio(ours, theirs), edges=int(graph[1].numel()),
                                          sweeps_mean=round(float(sweeps.float().mean()), 1), sweeps_max=int(sweeps.max()))

    # ---- 12 500 vertices -> 1 024 samples: nearest + weights
    pos, face, graph, samples = mesh_on(12500, 2, dev, 1024)
    _, _, sweeps = G.nearest_sample(pos, face, samples, graph=graph, return_sweeps=True)
    ours = device_ms(lambda: G.sample_weights(pos, face, samples, graph=graph), args.warmup, args.reps)
    sg = scipy_graph(graph, 12500)
    mass = G.vertex_masses(pos, face).double().cpu().numpy()
    src = samples.cpu().numpy()

    def scipy_weights():
        _, _, nearest = dijkstra(sg, indices=src, min_only=True, return_predecessors=True)
        w = np.zeros(12500)
        np.add.at(w, nearest, mass)
        return w
    theirs = host_ms(scipy_weights, args.scipy_reps)
    res['cases']['nearest_weights_12500_to_1024'] = dict(device=ours, scipy=theirs, device_over_scipy=ratio(ours, theirs),
                                                         sweeps=sweeps[0].tolist())

    # ---- 8 such meshes: one batched call against 8 single calls
    meshes = [mesh_on(12500, 10 + b, dev, 1024) for b in range(8)]
    bpos = torch.cat([m[0] for m in meshes])
    bface = torch.cat([m[1] + 12500 * b for b, m in enumerate(meshes)], 1)
    bsamples = torch.cat([m[3] + 12500 * b for b, m in enumerate(meshes)])
    pos_ptr = torch.arange(9) * 12500
    sample_ptr = torch.arange(9) * 1024
    bgraph = G.mesh_edge_graph(bpos, bface)
    _, _, sweeps = G.nearest_sample(bpos, bface, bsamples, pos_ptr, sample_ptr, graph=bgraph, return_sweeps=True)
    batched = device_ms(lambda: G.sample_weights(bpos, bface, bsamples, pos_ptr, sample_ptr, graph=bgraph), args.warmup, args.reps)
    singles = device_ms(lambda: [G.sample_weights(m[0], m[1], m[3], graph=m[2]) for m in meshes], args.warmup, args.reps)
    res['cases']['batch_8x12500_to_1024'] = dict(batched=batched, eight_single_calls=singles, batched_over_singles=ratio(batched, singles),
                                                 sweeps_max=sweeps.max(0).values.tolist())

    # ---- one 160 000-vertex mesh: the one-workgroup global-memory path
    pos, face, graph, samples = mesh_on(160000, 3, dev, 1024)
    _, _, sweeps = G.nearest_sample(pos, face, samples, graph=graph, return_sweeps=True)
    ours = device_ms(lambda: G.nearest_sample(pos, face, samples, graph=graph), args.warmup, args.reps)
    sg = scipy_graph(graph, 160000)
    src = samples.cpu().numpy()
    theirs = host_ms(lambda: dijkstra(sg, indices=src, min_only=True, return_predecessors=True), args.scipy_reps)
    res['cases']['nearest_160000_to_1024_global_path'] = dict(device=ours, scipy=theirs, device_over_scipy=ratio(ours, theirs),
                                                              sweeps=sweeps[0].tolist())

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
