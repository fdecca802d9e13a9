#!/usr/bin/env python3
"""Max pooling by magnitude (fieldconv_amd.transfer.tangent_transfer_max, fieldconv_amd.pooling.mesh_max, csrc/fc_maxpool.hip)
beside the stock-op composite on the same device in the same run (not part of bench.py).

    level pairs     12 500 -> 1 024 and 20 000 -> 2 500 samples, the levels of tools/transfer_throughput.py; tangent_transfer_max on
                    the pool plan, complex64, C = 48 and 64, forward and forward + backward
    meshes          mesh_max at 8 meshes of 1 024 rows and at one mesh of 20 000 rows, complex64, C = 48 and 64
    composite       tangent_transfer_max: abs, scatter_reduce(..., 'amax'), an equality mask, a second scatter_reduce ('amin' of the
                    slot numbers: the tie rule), a gather and a multiply.  mesh_max: a shorter one -- abs, the origin-box mask and
                    one scatter_reduce(..., 'amax'); it yields no winner and has no tie rule, and its backward splits the gradient
                    among tied rows.  Autograd for the backward of both

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
No time is gated.  Writes one JSON object (--out).

    python tools/maxpool_throughput.py --out profiles/maxpool_throughput.json
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


def transfer_composite(x, n_out, out, inn, unit):
    """max by magnitude over the rows [out, in] with stock ops: the first slot of the largest |x| per (output row, channel)"""
    E, C = int(out.numel()), int(x.shape[1])
    v = x[inn]
    mag = v.abs()
    where = out[:, None].expand(E, C)
    top = torch.zeros(n_out, C, dtype=mag.dtype, device=x.device).scatter_reduce(0, where, mag, 'amax', include_self=False)
    slot = torch.where(mag == top[out], torch.arange(E, device=x.device)[:, None], E)
    first = torch.full((n_out, C), E, device=x.device).scatter_reduce(0, where, slot, 'amin')
    have = first < E
    sel = first.clamp(max=E - 1)
    return torch.where(have, unit[sel] * torch.gather(v, 0, sel), 0)


def mesh_composite(x, batch, B):
    mag = x.abs()
    mag = torch.where((x.real.abs() < 1e-7) & (x.imag.abs() < 1e-7), 0, mag)
    return torch.zeros(B, x.shape[1], dtype=mag.dtype, device=x.device).scatter_reduce(0, batch[:, None].expand_as(mag), mag, 'amax',
                                                                                      include_self=False)


def both(op, x, g, warmup, reps):
    """forward and forward + backward of op on x"""
    xg = x.clone().requires_grad_(True)
    return (device_ms(lambda: op(x), warmup, reps),
            device_ms(lambda: torch.autograd.grad(op(xg), xg, g), warmup, reps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('maxpool_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.pooling import mesh_max, tag_ptr
    from fieldconv_amd.transfer import tangent_transfer_max
    from fieldconv_amd.transforms import CoarsenSamples, ComputeLogXPort, GeodesicSupportGraph
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), cases={})

    def measure(ours, theirs, x, g):
        y, y_ref = ours(x), theirs(x)
        r = dict(max_abs_difference_from_composite=float((y - y_ref).abs().max()))
        r['forward'], r['forward_backward'] = both(ours, x, g, args.warmup, args.reps)
        r['forward_composite'], r['forward_backward_composite'] = both(theirs, x, g, args.warmup, args.reps)
        r['forward_ratio'] = ratio(r['forward'], r['forward_composite'])
        r['forward_backward_ratio'] = ratio(r['forward_backward'], r['forward_backward_composite'])
        return r

    for V, S_c, seed in ((12500, 1024, 2), (20000, 2500, 3)):
        pos, face = (t.to(dev) for t in surface(V, seed))
        eps_f, eps_c = math.sqrt(32 / (math.pi * V)), math.sqrt(32 / (math.pi * S_c))          # about 32 neighbours on a unit-area sheet
        data = SimpleNamespace(pos=pos, face=face, sample_idx=torch.arange(V, device=dev))
        plan = CoarsenSamples(S_c, eps_c)(ComputeLogXPort(eps_f)(GeodesicSupportGraph(eps_f)(data))).pool
        rows, _, phase = plan.rows()
        unit = (phase.conj() if plan.conj_phase else phase).resolve_conj()
        out, inn = rows[:, 0].contiguous(), rows[:, 1].contiguous()
        case = dict(fine_samples=V, coarse_samples=S_c, rows=plan.n_rows)
        for C in (48, 64):
            x = torch.randn(plan.n_in, C, dtype=torch.complex64, device=dev)
            g = torch.randn(plan.n_out, C, dtype=torch.complex64, device=dev)
            case[f'C{C}'] = measure(lambda t: tangent_transfer_max(t, plan), lambda t: transfer_composite(t, plan.n_out, out, inn, unit), x, g)
        res['cases'][f'transfer_max_{V}_to_{S_c}'] = case

    for B, n in ((8, 1024), (1, 20000)):
        ptr = tag_ptr((torch.arange(B + 1, dtype=torch.int64) * n).to(dev), range(0, (B + 1) * n, n))          # as a MeshBatch's: no synchronisation
        batch = torch.arange(B, device=dev).repeat_interleave(n)
        case = dict(meshes=B, rows_per_mesh=n)
        for C in (48, 64):
            x = torch.randn(B * n, C, dtype=torch.complex64, device=dev)
            g = torch.randn(B, C, device=dev)
            case[f'C{C}'] = measure(lambda t: mesh_max(t, ptr), lambda t: mesh_composite(t, batch, B), x, g)
        res['cases'][f'mesh_max_{B}x{n}'] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
