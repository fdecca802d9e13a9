#!/usr/bin/env python3
"""Geodesic farthest-point sampling and geodesic-ball support edges (fieldconv_amd.geodesic_sampling) against what the package
could do before them on the same device, and against scipy.sparse.csgraph.dijkstra on the same box and graph (not part of
bench.py).

    fps         12 500 vertices -> 1 024 samples: one launch, against a Python loop of nearest_sample + argmax (one launch and
                one host round trip per sample; the loop takes the first of the largest, which is the same selection where no
                vertex holds d = 0 without being taken) and against scipy (min_only Dijkstra from all samples so far + argmax)
    fps_batch   8 such meshes as one batched call against 8 single calls
    ball        the support edges of those 1 024 samples at epsilon = 0.2, and of ALL 4 999 vertices of a 4 999-vertex mesh at
                epsilon = 0.0425, against geodesic_distances rows + a threshold (device) and scipy's dijkstra with limit=epsilon

Meshes: random points of the unit square, Delaunay-triangulated and lifted by a smooth height.  The edge graph is built once per
mesh and passed in (graph=): what is timed is the solve, its launches and its torch glue.  Device events around each repetition
after a common warm-up, median of --reps (5); scipy by perf_counter, median of --scipy-reps; the slow baselines (the loop, scipy's
sampling) run --slow-reps times.  Sweep counts are recorded beside the times.  Writes one JSON object (--out).

    python tools/geodesic_sampling_throughput.py --out profiles/geodesic_sampling_throughput.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, host_ms, ratio, scipy_graph, surface          # noqa: E402  (the same protocol)


def mesh_on(n, seed, dev):
    from fieldconv_amd.geodesic import mesh_edge_graph
    pos, face = surface(n, seed)
    pos, face = pos.to(dev), face.to(dev)
    return pos, face, mesh_edge_graph(pos, face)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--scipy-reps', type=int, default=3)
    ap.add_argument('--slow-reps', type=int, default=1)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('geodesic_sampling_throughput.py measures on a ROCm device and none is visible')
    from scipy.sparse.csgraph import dijkstra
    from fieldconv_amd import geodesic as G
    from fieldconv_amd import geodesic_sampling as GS
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), lds_vertices=GS.LDS_VERTICES, cases={})
    V, S = 12500, 1024

    # ---- sampling: 12 500 vertices -> 1 024 samples
    pos, face, graph = mesh_on(V, 2, dev)
    idx, dist, sweeps = GS.geodesic_farthest_point_sample(pos, face, S, 0, graph=graph, return_dist=True, return_sweeps=True)
    ours = device_ms(lambda: GS.geodesic_farthest_point_sample(pos, face, S, 0, graph=graph), args.warmup, args.reps)

    def loop():
        taken = torch.zeros(S, dtype=torch.int64, device=dev)
        for k in range(1, S):
            d = G.nearest_sample(pos, face, taken[:k], graph=graph)[1]
            taken[k] = int(torch.argmax(d))          # the host round trip a composition cannot avoid: the next call's sources
        return taken
    same = bool(torch.equal(loop(), idx))
    before = device_ms(loop, 0, args.slow_reps)
    sg = scipy_graph(graph, V)

    def scipy_fps():
        taken = [0]
        for _ in range(1, S):
            taken.append(int(np.argmax(dijkstra(sg, indices=taken, min_only=True))))
        return taken
    theirs = host_ms(scipy_fps, args.slow_reps)
    res['cases']['fps_12500_to_1024'] = dict(
        device=ours, nearest_sample_loop=before, scipy=theirs, device_over_loop=ratio(ours, before), device_over_scipy=ratio(ours, theirs),
        loop_gives_the_same_samples=same, sweeps_total=int(sweeps), sweeps_per_round=round(int(sweeps) / S, 2),
        covering_radius=round(float(dist.max()), 6))

    # ---- 8 such meshes: one batched call against 8 single calls
    meshes = [mesh_on(V, 10 + b, dev) for b in range(8)]
    bpos = torch.cat([m[0] for m in meshes])
    bface = torch.cat([m[1] + V * b for b, m in enumerate(meshes)], 1)
    pos_ptr = torch.arange(9) * V
    bgraph = G.mesh_edge_graph(bpos, bface)
    _, bsweeps = GS.geodesic_farthest_point_sample_batched(bpos, bface, pos_ptr, S, graph=bgraph, return_sweeps=True)
    batched = device_ms(lambda: GS.geodesic_farthest_point_sample_batched(bpos, bface, pos_ptr, S, graph=bgraph), args.warmup, args.reps)
    singles = device_ms(lambda: [GS.geodesic_farthest_point_sample(m[0], m[1], S, graph=m[2]) for m in meshes], args.warmup, args.reps)
    res['cases']['fps_batch_8x12500_to_1024'] = dict(batched=batched, eight_single_calls=singles, batched_over_singles=ratio(batched, singles),
                                                     sweeps_total_max=int(bsweeps.max()))

    # ---- ball edges
    def ball_case(name, pos, face, graph, samples, eps):
        n = int(pos.shape[0])
        edges = GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph)
        ours = device_ms(lambda: GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph), args.warmup, args.reps)

        def rows_then_threshold():
            rows = G.geodesic_distances(pos, face, samples, graph=graph)[:, samples]
            return torch.nonzero(rows < eps)
        same = bool(torch.equal(rows_then_threshold(), edges))
        _, row_sweeps = G.geodesic_distances(pos, face, samples, graph=graph, return_sweeps=True)
        before = device_ms(rows_then_threshold, args.warmup, args.reps)
        sg, src = scipy_graph(graph, n), samples.cpu().numpy()

        def scipy_ball():
            rows = dijkstra(sg, indices=src, limit=eps)[:, src]
            return np.argwhere(rows < eps)
        theirs = host_ms(scipy_ball, args.scipy_reps)
        res['cases'][name] = dict(device=ours, rows_then_threshold=before, scipy_limit=theirs, device_over_rows=ratio(ours, before),
                                  device_over_scipy=ratio(ours, theirs), rows_give_the_same_edges=same, edges=int(edges.shape[0]),
                                  edges_per_query=round(edges.shape[0] / samples.numel(), 1),
                                  unbounded_row_sweeps_mean=round(float(row_sweeps.float().mean()), 1))

    ball_case('ball_1024_of_12500_eps_0.2', pos, face, graph, idx.sort()[0], 0.2)
    pos, face, graph = mesh_on(4999, 1, dev)
    ball_case('ball_4999_of_4999_eps_0.0425', pos, face, graph, torch.arange(4999, device=dev), 0.0425)

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
