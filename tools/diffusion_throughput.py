#!/usr/bin/env python3
"""Heat diffusion of sample features (fieldconv_amd.diffusion, csrc/fc_diffusion.hip) beside the same recurrence composed of stock
ops on the same device in the same run (not part of bench.py).

    levels          of the 12 500-vertex mesh of tools/geodesic_throughput.py: its 1 024-sample level (geodesic farthest-point
                    sampling, epsilon for about 40 rows per sample), a batch of 8 such levels (the level's rows side by side, one ptr),
                    and all 12 500 vertices as samples; GeodesicSupportGraph + ComputeLogXPort + DiffusionOperator
    cases           heat_diffuse forward and forward + backward (torch.autograd.grad to x and t), complex64, iters = 16, C = 48 and 64
    composite       the recurrence of include/fieldconv_hip.h with index_select, multiply, index_add_ and sum per iteration, float32
                    inner products, no fixed order; its backward is the same implicit one (a second composite solve and one product)
    residual        sqrt(<r, z>) at exit, the largest over meshes and channels, for iters in 4, 8, 16, 32

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
Writes one JSON object (--out).

    python tools/diffusion_throughput.py --out profiles/diffusion_throughput.json
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


def composite_solver(plan, ptr):
    """the stock-op recurrence on the plan's own entries -> solve(rhs_is_wx, x, t, iters) -> y"""
    dev, n = plan.device, plan.n
    row = torch.repeat_interleave(torch.arange(n, device=dev), (plan.rowptr[1:] - plan.rowptr[:-1]).to(torch.int64))
    col, coef, d, w = plan.col.to(torch.int64), plan.coef, plan.diag[:, None], plan.w[:, None]
    B = ptr.numel() - 1
    mesh = torch.repeat_interleave(torch.arange(B, device=dev), ptr[1:] - ptr[:-1])

    def A(v, t):
        sx = torch.zeros_like(v).index_add_(0, row, coef[:, None] * v.index_select(0, col)) + d * v
        return w * v + t * sx

    def dot(u, v):
        return torch.zeros(B, u.shape[1], device=dev).index_add_(0, mesh, (u.conj() * v).real).index_select(0, mesh)

    def solve(forward, x, t, iters):
        P = w + t * d
        y, rhs = (x, w * x) if forward else (x / w, x)
        r = rhs - A(y, t)
        z = r / P
        p, rz = z, dot(r, z)
        for _ in range(iters):
            q = A(p, t)
            pq = dot(p, q)
            alpha = torch.where(pq > 0, rz / pq, torch.zeros_like(pq))
            y, r = y + alpha * p, r - alpha * q
            z = r / P
            rz_new = dot(r, z)
            beta = torch.where(rz > 0, rz_new / rz, torch.zeros_like(rz))
            p, rz = z + beta * p, rz_new
        return y if forward else w * y

    def forward_backward(x, t, gy, iters):
        y = solve(True, x, t, iters)
        gx = solve(False, gy, t, iters)
        lam = gx / w
        sy = torch.zeros_like(y).index_add_(0, row, coef[:, None] * y.index_select(0, col)) + d * y
        return y, gx, -(lam.conj() * sy).real.sum(0)
    return solve, forward_backward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('diffusion_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.diffusion import diffusion_plan, heat_diffuse
    from fieldconv_amd.transforms import ComputeLogXPort, DiffusionOperator, GeodesicSupportGraph
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), iters=16, cases={})
    V = 12500
    pos, face = (t.to(dev) for t in surface(V, 2))

    def level(samples):
        eps = math.sqrt(52 / (math.pi * samples))          # about 40 rows per sample on the unit square, less the balls the border cuts
        data = SimpleNamespace(pos=pos, face=face)
        data = GeodesicSupportGraph(eps, sample_n=samples if samples < V else None, random_start=False)(data)
        return DiffusionOperator()(ComputeLogXPort(eps)(data)), eps

    small, eps_small = level(1024)
    big, eps_big = level(V)
    S = small.diffusion_plan.n
    shift = (torch.arange(8, device=dev) * S).repeat_interleave(small.supp_edges.shape[0])[:, None]
    batch_plan = diffusion_plan(small.supp_edges.repeat(8, 1) + shift, small.xp.repeat(8), small.logMag.repeat(8), 8 * S,
                                small.w.reshape(-1).repeat(8), small.diffusion_plan.h)
    levels = (('1024', small.diffusion_plan, torch.tensor([0, S], device=dev), eps_small),
              ('8x1024', batch_plan, torch.arange(9, device=dev) * S, eps_small),
              ('12500', big.diffusion_plan, torch.tensor([0, V], device=dev), eps_big))
    for name, plan, ptr, eps in levels:
        n = plan.n
        d = plan.diag
        t_scale = float(plan.w.median() / d[d > 0].median())          # t d ~ w: the diffusion term as large as the mass term
        case = dict(samples=n, meshes=ptr.numel() - 1, epsilon=round(eps, 5), entries=plan.n_entries, entries_per_row=round(plan.n_entries / n, 1),
                    h=plan.h, time_scale=t_scale)
        solve, forward_backward = composite_solver(plan, ptr)
        use_ptr = ptr if ptr.numel() > 2 else None
        for C in (48, 64):
            x = torch.randn(n, C, dtype=torch.complex64, device=dev)
            gy = torch.randn(n, C, dtype=torch.complex64, device=dev)
            t = t_scale * torch.linspace(0.25, 4.0, C, device=dev)
            xg, tg = x.clone().requires_grad_(True), t.clone().requires_grad_(True)
            y, y_ref = heat_diffuse(x, t, plan, ptr=use_ptr, iters=16), solve(True, x, t[None, :], 16)
            r = dict(max_abs_difference_from_composite=float((y - y_ref).abs().max()), largest_entry=float(y_ref.abs().max()))
            r['forward'] = device_ms(lambda: heat_diffuse(x, t, plan, ptr=use_ptr, iters=16), args.warmup, args.reps)
            r['forward_composite'] = device_ms(lambda: solve(True, x, t[None, :], 16), args.warmup, args.reps)
            r['forward_backward'] = device_ms(lambda: torch.autograd.grad(heat_diffuse(xg, tg, plan, ptr=use_ptr, iters=16), [xg, tg], gy),
                                              args.warmup, args.reps)
            r['forward_backward_composite'] = device_ms(lambda: forward_backward(x, t[None, :], gy, 16), args.warmup, args.reps)
            for what in ('forward', 'forward_backward'):
                r[what + '_ratio'] = ratio(r[what], r[what + '_composite'])
            r['residual_at_exit'] = {str(k): float(heat_diffuse(x, t, plan, ptr=use_ptr, iters=k, return_residual=True)[1].max())
                                     for k in (4, 8, 16, 32)}
            case[f'C{C}'] = r
        res['cases'][name] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
