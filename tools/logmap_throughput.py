#!/usr/bin/env python3
"""Log map and parallel transport on the device (fieldconv_amd.logmap) beside the ball search it grows from, on the meshes of
tools/geodesic_sampling_throughput.py (not part of bench.py).

    logmap      12 500 vertices, 1 024 geodesic-FPS samples, the support edges of GeodesicSupportGraph at epsilon = 0.2 and
                bound = 0.2: log_map_transport (frames, trees, unfolding, rows) against geodesic_radius_edges on the same
                samples (the same relaxation, solved twice, and nothing after it), with the LDS ball state and with every ball
                in its workspace slot
    frames      vertex_frames of that mesh alone
    all_of_4999 all 4 999 vertices of a 4 999-vertex mesh at epsilon = bound = 0.0425

The edge graph is built once per mesh and passed in (graph=).  Device events around each repetition after a common warm-up,
median of --reps (5): the protocol of tools/geodesic_throughput.py.  There is no host baseline: scipy has no unfolding, and the
numpy restatement of the tests is a definition, not a competitor.  Writes one JSON object (--out).

    python tools/logmap_throughput.py --out profiles/logmap_throughput.json
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, ratio          # noqa: E402  (the same protocol)
from geodesic_sampling_throughput import mesh_on          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('logmap_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd import geodesic_sampling as GS
    from fieldconv_amd import logmap as LM
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), ball_lds_vertices=LM.BALL_LDS_VERTICES, cases={})

    def case(name, pos, face, graph, samples, eps):
        edges = GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph)
        out = LM.log_map_transport(pos, face, samples, edges, eps, graph=graph, return_reached=True)
        ours = device_ms(lambda: LM.log_map_transport(pos, face, samples, edges, eps, graph=graph), args.warmup, args.reps)
        slots = device_ms(lambda: LM.log_map_transport(pos, face, samples, edges, eps, graph=graph, ball_lds_vertices=0), args.warmup, args.reps)
        balls = device_ms(lambda: GS.geodesic_radius_edges(pos, face, samples, eps, graph=graph), args.warmup, args.reps)
        res['cases'][name] = dict(log_map_transport=ours, with_every_ball_in_its_workspace_slot=slots, geodesic_radius_edges=balls,
                                  logmap_over_ball_search=ratio(ours, balls), slots_over_lds=ratio(slots, ours), rows=int(edges.shape[0]),
                                  rows_per_query=round(edges.shape[0] / samples.numel(), 1), every_row_reached=bool(out[3].all()))

    pos, face, graph = mesh_on(12500, 2, dev)
    samples = GS.geodesic_farthest_point_sample(pos, face, 1024, 0, graph=graph).sort()[0]
    case('logmap_1024_of_12500_eps_0.2', pos, face, graph, samples, 0.2)
    res['cases']['frames_12500'] = dict(vertex_frames=device_ms(lambda: LM.vertex_frames(pos, face), args.warmup, args.reps))
    pos, face, graph = mesh_on(4999, 1, dev)
    case('logmap_4999_of_4999_eps_0.0425', pos, face, graph, torch.arange(4999, device=dev), 0.0425)

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
