#!/usr/bin/env python3
"""What the unfolded diagonals of mesh_edge_graph(pos, face, diagonals=True) cost: building the graph, and every solver that
runs over it, on the side graph and on the enriched one (not part of bench.py).

    graph       mesh_edge_graph with and without diagonals at 12 500 and 160 000 vertices (the sort, the two kernels of
                csrc/fc_mesh_graph.hip and the torch glue around them)
    consumers   the 12 500-vertex mesh, each graph built once and passed in (graph=): nearest_sample of 1 024 samples, geodesic
                farthest-point sampling of 1 024 samples, geodesic_radius_edges and log_map_transport of those samples at
                epsilon = bound = 0.2, with the sweep counts where the call reports them.  Each graph takes its own samples and
                support edges: that is what a pipeline run with diagonals=True does.

Meshes are those of tools/geodesic_throughput.py.  Device events around each repetition after a common warm-up, median of --reps
(5): the protocol of that tool.  Every time on the enriched graph is also given as a ratio to the side graph's.  Writes one JSON
object (--out).

    python tools/edge_graph_throughput.py --out profiles/edge_graph_throughput.json
"""
import argparse
import json
import os
import sys

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
        raise SystemExit('edge_graph_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd import geodesic as G
    from fieldconv_amd import geodesic_sampling as GS
    from fieldconv_amd import logmap as LM
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), cases={})
    ms = lambda fn: device_ms(fn, args.warmup, args.reps)

    def both(side, rich, **extra):
        return dict(side_graph=side, with_diagonals=rich, diagonals_over_side=ratio(rich, side), **extra)

    # ---- building the graph
    meshes = {}
    for n, seed in ((12500, 2), (160000, 3)):
        pos, face = surface(n, seed)
        pos, face = pos.to(dev), face.to(dev)
        graphs = [G.mesh_edge_graph(pos, face, diagonals=d) for d in (False, True)]
        meshes[n] = (pos, face, graphs)
        res['cases'][f'mesh_edge_graph_{n}'] = both(ms(lambda: G.mesh_edge_graph(pos, face)), ms(lambda: G.mesh_edge_graph(pos, face, diagonals=True)),
                                                    faces=int(face.shape[1]), directed_edges_side=int(graphs[0][1].numel()),
                                                    directed_edges_with_diagonals=int(graphs[1][1].numel()))

    # ---- the solvers over each graph
    pos, face, graphs = meshes[12500]
    S, eps = 1024, 0.2
    times = {name: [] for name in ('nearest_sample', 'geodesic_fps', 'geodesic_radius_edges', 'log_map_transport')}
    notes = {name: [] for name in times}
    for graph in graphs:
        idx, dist, sweeps = GS.geodesic_farthest_point_sample(pos, face, S, 0, graph=graph, return_dist=True, return_sweeps=True)
        times['geodesic_fps'].append(ms(lambda: GS.geodesic_farthest_point_sample(pos, face, S, 0, graph=graph)))
        notes['geodesic_fps'].append(dict(sweeps_total=int(sweeps), covering_radius=round(float(dist.max()), 6)))
        samples = idx.sort()[0]
        near = G.nearest_sample(pos, face, samples, graph=graph, return_sweeps=True)[2]
        times['nearest_sample'].append(ms(lambda: G.nearest_sample(pos, face, samples, graph=graph)))
        notes['nearest_sample'].append(dict(distance_sweeps=int(near[0, 0]), label_sweeps=int(near[0, 1])))
        edges = GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph)
        times['geodesic_radius_edges'].append(ms(lambda: GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph)))
        notes['geodesic_radius_edges'].append(dict(edges=int(edges.shape[0]), edges_per_query=round(edges.shape[0] / S, 1)))
        reached = LM.log_map_transport(pos, face, samples, edges, eps, graph=graph, return_reached=True)[3]
        times['log_map_transport'].append(ms(lambda: LM.log_map_transport(pos, face, samples, edges, eps, graph=graph)))
        notes['log_map_transport'].append(dict(rows=int(edges.shape[0]), every_row_reached=bool(reached.all())))
    for name in times:
        res['cases'][f'{name}_1024_of_12500'] = both(*times[name], side_graph_notes=notes[name][0], with_diagonals_notes=notes[name][1])

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
