#!/usr/bin/env python3
"""The intrinsic gradient and Laplacian of sample features (fieldconv_amd.diffops, csrc/fc_diffops.hip) beside the stock composite
on the same device in the same run (not part of bench.py).

    levels          every vertex of a 12 500- and of a 20 000-vertex mesh of tools/geodesic_throughput.py as a sample, epsilon chosen
                    for about 85 rows per query; GeodesicSupportGraph + ComputeLogXPort + GradientOperator
    operators       tangent_gradient forward, forward + backward (torch.autograd.grad), and laplacian forward; float32, C = 48 and 64
    composite       index_select of both ends of every row, a subtract, a multiply by the plan's own coefficients, index_add_ onto
                    the query rows; its backward is autograd's; its Laplacian applies the same four steps in the other direction
    plan            gradient_plan itself (two sorts and fc_gradient_coefficients)

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
Writes one JSON object (--out).

    python tools/diffops_throughput.py --out profiles/diffops_throughput.json
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
        raise SystemExit('diffops_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.diffops import gradient_plan, laplacian, tangent_gradient
    from fieldconv_amd.transforms import ComputeLogXPort, GeodesicSupportGraph, GradientOperator
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), cases={})

    for V, seed in ((12500, 2), (20000, 3)):
        pos, face = (t.to(dev) for t in surface(V, seed))
        eps = math.sqrt(111 / (math.pi * V))          # about 85 rows per query: 111 on an unbounded sheet, less the balls the border cuts
        data = SimpleNamespace(pos=pos, face=face, sample_idx=torch.arange(V, device=dev))
        data = GradientOperator()(ComputeLogXPort(eps)(GeodesicSupportGraph(eps)(data)))
        plan = data.grad_plan
        w = plan.w
        query = torch.repeat_interleave(torch.arange(V, device=dev), (plan.rowptr[1:] - plan.rowptr[:-1]).to(torch.int64))
        col, coef = plan.col.to(torch.int64), plan.coef
        case = dict(samples=V, epsilon=round(eps, 5), rows=plan.n_slots, rows_per_query=round(plan.n_slots / V, 1),
                    invalid_rows=int(plan.n_invalid))
        case['gradient_plan'] = device_ms(lambda: gradient_plan(data.supp_edges, data.logMag, data.logAng, V, w), args.warmup, args.reps)

        def composite_gradient(x):
            d = x.index_select(0, col) - x.index_select(0, query)
            return torch.zeros(V, x.shape[1], dtype=torch.complex64, device=dev).index_add_(0, query, coef[:, None] * d)

        def composite_laplacian(x):
            t = (coef[:, None].conj() * (w[:, None] * composite_gradient(x)).index_select(0, query)).real
            out = torch.zeros(V, x.shape[1], device=dev).index_add_(0, col, t).index_add_(0, query, -t)
            return out * (-1.0 / w)[:, None]

        for C in (48, 64):
            x = torch.randn(V, C, device=dev)
            gy = torch.randn(V, C, dtype=torch.complex64, device=dev)
            xg = x.clone().requires_grad_(True)
            y, y_ref = tangent_gradient(x, plan), composite_gradient(x)
            lap, lap_ref = laplacian(x, plan), composite_laplacian(x)
            r = dict(max_abs_difference_from_composite=float((y - y_ref).abs().max()), largest_entry=float(y_ref.abs().max()),
                     laplacian_max_abs_difference_from_composite=float((lap - lap_ref).abs().max()),
                     laplacian_largest_entry=float(lap_ref.abs().max()))
            r['forward'] = device_ms(lambda: tangent_gradient(x, plan), args.warmup, args.reps)
            r['forward_composite'] = device_ms(lambda: composite_gradient(x), args.warmup, args.reps)
            r['forward_backward'] = device_ms(lambda: torch.autograd.grad(tangent_gradient(xg, plan), xg, gy), args.warmup, args.reps)
            r['forward_backward_composite'] = device_ms(lambda: torch.autograd.grad(composite_gradient(xg), xg, gy), args.warmup, args.reps)
            r['laplacian'] = device_ms(lambda: laplacian(x, plan), args.warmup, args.reps)
            r['laplacian_composite'] = device_ms(lambda: composite_laplacian(x), args.warmup, args.reps)
            for name in ('forward', 'forward_backward', 'laplacian'):
                r[name + '_ratio'] = ratio(r[name], r[name + '_composite'])
            case[f'C{C}'] = r
        res['cases'][str(V)] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
