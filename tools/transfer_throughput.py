#!/usr/bin/env python3
"""Tangent-feature pooling and unpooling between two sample levels (fieldconv_amd.transfer, csrc/fc_transfer.hip) beside the
stock composite on the same device, and building a level beside building the fine level (not part of bench.py).

    level pairs     12 500 -> 1 024 samples of a 12 500-vertex mesh, 20 000 -> 2 500 of a 20 000-vertex mesh (the fine level is
                    every vertex; epsilon chosen for about 32 neighbours at each level), meshes of tools/geodesic_throughput.py
    transfer        pool and unpool, forward and backward (the kernel on the transposed CSR), complex64, C = 48 and 64, against
                    torch.zeros(n_out, C).index_add_(0, out, coef[:, None] * x[in]) with the same rows and coefficients
    build           transforms.CoarsenSamples (sampling, support edges, log map and weights of the coarse level, cells, both
                    plans) beside GeodesicSupportGraph + ComputeLogXPort of the fine level

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
Writes one JSON object (--out).

    python tools/transfer_throughput.py --out profiles/transfer_throughput.json
"""
import argparse
import json
import math
import os
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, ratio, surface          # noqa: E402  (the same protocol, the same meshes)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('transfer_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.transfer import tangent_transfer
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), cases={})

    for V, S_c, seed in ((12500, 1024, 2), (20000, 2500, 3)):
        pos, face = (t.to(dev) for t in surface(V, seed))
        eps_f, eps_c = math.sqrt(32 / (math.pi * V)), math.sqrt(32 / (math.pi * S_c))          # about 32 neighbours on a unit-area sheet

        def fine_level():
            data = SimpleNamespace(pos=pos, face=face, sample_idx=torch.arange(V, device=dev))
            return ComputeLogXPort(eps_f)(GeodesicSupportGraph(eps_f)(data))
        fine = fine_level()
        coarsen = CoarsenSamples(S_c, eps_c)
        level = coarsen(fine)
        case = dict(fine_samples=V, coarse_samples=S_c, epsilon_fine=round(eps_f, 5), epsilon_coarse=round(eps_c, 5),
                    fine_edges=int(fine.supp_edges.shape[0]), coarse_edges=int(level.supp_edges.shape[0]), outside=level.n_outside,
                    largest_cell=int(torch.bincount(level.cell[level.cell >= 0]).max()))
        case['build_fine_level'] = device_ms(fine_level, args.warmup, args.reps)
        case['coarsen_samples'] = device_ms(lambda: coarsen(fine), args.warmup, args.reps)
        case['coarsen_over_fine_level'] = ratio(case['coarsen_samples'], case['build_fine_level'])
        for C in (48, 64):
            for name, plan in (('pool', level.pool), ('unpool', level.unpool)):
                rows, weight, phase = plan.rows()
                coef = (weight * (phase.conj() if plan.conj_phase else phase)).resolve_conj()
                out, inn = rows[:, 0].contiguous(), rows[:, 1].contiguous()
                x = torch.randn(plan.n_in, C, dtype=torch.complex64, device=dev)
                gy = torch.randn(plan.n_out, C, dtype=torch.complex64, device=dev)
                adj, coef_h = plan.adjoint(), coef.conj().resolve_conj()

                def composite(v, n, o, i, c):
                    return torch.zeros(n, C, dtype=torch.complex64, device=dev).index_add_(0, o, c[:, None] * v[i])
                y, y_ref = tangent_transfer(x, plan), composite(x, plan.n_out, out, inn, coef)
                r = dict(rows=plan.n_rows, max_abs_difference_from_composite=float((y - y_ref).abs().max()))
                r['forward'] = device_ms(lambda: tangent_transfer(x, plan), args.warmup, args.reps)
                r['forward_composite'] = device_ms(lambda: composite(x, plan.n_out, out, inn, coef), args.warmup, args.reps)
                r['backward'] = device_ms(lambda: tangent_transfer(gy, adj), args.warmup, args.reps)
                r['backward_composite'] = device_ms(lambda: composite(gy, plan.n_in, inn, out, coef_h), args.warmup, args.reps)
                r['forward_ratio'], r['backward_ratio'] = ratio(r['forward'], r['forward_composite']), ratio(r['backward'], r['backward_composite'])
                case[f'{name}_C{C}'] = r
        res['cases'][f'{V}_to_{S_c}'] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
