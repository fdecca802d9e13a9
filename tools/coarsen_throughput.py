#!/usr/bin/env python3
"""What geodesic coarsening costs and what the restricted ball search saves (not part of bench.py), on the 12 500-vertex mesh
of tools/geodesic_throughput.py, edge graph built once and passed in (graph=):

    balls       geodesic_radius_edges(queries=coarse) for 1 024 of 12 500 samples (every vertex a fine sample) against the
                full call plus the filter of its rows, which is how interpolation_plan found its candidates before
    plan        interpolation_plan(k=3) at 12 500 -> 1 024 as it is now.  The previous revision is NOT timed here: the ball
                part above is the only before / after comparison
    sampling    geodesic farthest-point sampling of 1 024 among 4 096 candidates against the unrestricted 1 024 rounds
    coarsen     CoarsenSamples(1024, 0.4, sampling='geodesic') against sampling='euclidean' on a 4 096-sample fine level

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of geodesic_throughput.py.
Writes one JSON object (--out).

    python tools/coarsen_throughput.py --out profiles/coarsen_throughput.json
"""
import argparse
import json
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, ratio, surface          # noqa: E402  (the same protocol)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('coarsen_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd import geodesic as G
    from fieldconv_amd import geodesic_sampling as GS
    from fieldconv_amd.transfer import interpolation_plan
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), cases={})
    ms = lambda fn: device_ms(fn, args.warmup, args.reps)
    pos, face = surface(12500, 2)
    pos, face = pos.to(dev), face.to(dev)
    V = int(pos.shape[0])
    graph = G.mesh_edge_graph(pos, face)
    every = torch.arange(V, device=dev)

    # ---- balls for the coarse queries only
    coarse = GS.geodesic_farthest_point_sample(pos, face, 1024, 0, graph=graph).sort()[0]          # positions = vertices: every vertex is a sample
    far = float(G.nearest_sample(pos, face, coarse, graph=graph)[1].max())
    radius = 2.0 * far          # what interpolation_plan searches with

    def full_then_filter():
        edges = GS.geodesic_radius_edges(pos, face, every, radius, max_num_neighbors=V, graph=graph)
        where = torch.full((V,), -1, dtype=torch.int64, device=dev)
        where[coarse] = torch.arange(1024, device=dev)
        return edges[where[edges[:, 0]] >= 0]

    def listed():
        return GS.geodesic_radius_edges(pos, face, every, radius, max_num_neighbors=V, graph=graph, queries=coarse)
    same = torch.equal(full_then_filter(), listed())
    before, after = ms(full_then_filter), ms(listed)
    res['cases']['ball_edges_1024_of_12500'] = dict(all_queries_then_filter=before, queries_listed=after, listed_over_all=ratio(after, before),
                                                    radius=round(radius, 6), rows=int(listed().shape[0]), same_rows=same)

    # ---- the plan that uses them
    plan = interpolation_plan(pos, face, every, coarse, 3, graph=graph)
    res['cases']['interpolation_plan_k3_12500_to_1024'] = dict(now=ms(lambda: interpolation_plan(pos, face, every, coarse, 3, graph=graph)),
                                                                rows=int(plan.n_rows), previous_revision='not timed: see ball_edges_1024_of_12500')

    # ---- sampling among candidates
    fine = GS.geodesic_farthest_point_sample(pos, face, 4096, 0, graph=graph).sort()[0]
    start = int(fine[0])
    _, d_among, sw_among = GS.geodesic_farthest_point_sample(pos, face, 1024, start, graph=graph, candidates=fine, return_dist=True,
                                                             return_sweeps=True)
    _, d_all, sw_all = GS.geodesic_farthest_point_sample(pos, face, 1024, start, graph=graph, return_dist=True, return_sweeps=True)
    among = ms(lambda: GS.geodesic_farthest_point_sample(pos, face, 1024, start, graph=graph, candidates=fine))
    unrestricted = ms(lambda: GS.geodesic_farthest_point_sample(pos, face, 1024, start, graph=graph))
    res['cases']['geodesic_fps_1024_of_12500'] = dict(among_4096_candidates=among, every_vertex=unrestricted, among_over_every=ratio(among, unrestricted),
                                                      sweeps_among=int(sw_among), sweeps_every=int(sw_all),
                                                      covering_radius_among=round(float(d_among.max()), 6),
                                                      covering_radius_every=round(float(d_all.max()), 6))

    # ---- the transform
    level = SimpleNamespace(pos=pos, face=face, sample_idx=fine)
    level = ComputeLogXPort(0.05)(GeodesicSupportGraph(0.05)(level))
    rules = {}
    for rule in ('geodesic', 'euclidean'):
        rules[rule] = device_ms(lambda: CoarsenSamples(1024, 0.4, sampling=rule)(level), 1, args.reps)
    res['cases']['coarsen_samples_1024_of_4096'] = dict(geodesic=rules['geodesic'], euclidean=rules['euclidean'],
                                                        geodesic_over_euclidean=ratio(rules['geodesic'], rules['euclidean']))

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
