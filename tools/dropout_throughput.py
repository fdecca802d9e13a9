#!/usr/bin/env python3
"""tangent_dropout (fieldconv_amd.dropout, csrc/fc_dropout.hip) and RandomMeshAffine (fieldconv_amd.transforms, csrc/fc_augment.hip)
beside stock torch ops on the same device (not part of bench.py).

    dropout     complex64, p = 0.5, (12 500, 48) and (20 000, 64), element mode, the step in a device tensor (as nn.TangentDropout
                holds it); forward, and forward + backward (the gradient to x)
    composite   x * torch.nn.functional.dropout(torch.ones(N, C, device=...), p): a real mask from torch's own generator times
                the complex features; autograd for its backward
    augment     RandomMeshAffine(scale=(0.85, 1.15), center=True) on a MeshBatch of 8 meshes of 12 500 vertices, against the loop
                over batch.mesh(b) that does what the stock host transforms do with torch ops: subtract the mean, multiply by a
                scale drawn on the host, and three matrix products with rotation matrices built on the host

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
Writes one JSON object (--out).  Nothing is gated; box-to-box noise is +-5 %.

    python tools/dropout_throughput.py --out profiles/dropout_throughput.json
"""
import argparse
import json
import math
import os
import random
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, ratio          # noqa: E402  (the same protocol)


def rotation(axis, radians, device):
    """the matrix of the stock RandomRotate about one axis, built on the host and copied over"""
    c, s = math.cos(radians), math.sin(radians)
    m = ([[1, 0, 0], [0, c, s], [0, -s, c]], [[c, 0, -s], [0, 1, 0], [s, 0, c]], [[c, s, 0], [-s, c, 0], [0, 0, 1]])[axis]
    return torch.tensor(m, dtype=torch.float32, device=device)


def loop_augment(batch, scale, degrees, rng):
    """mesh by mesh with torch ops: Center, RandomScale and three RandomRotate, as the host transforms do them"""
    out = []
    for b in range(batch.num_meshes):
        pos = batch.mesh(b).pos
        pos = pos - pos.mean(dim=0, keepdim=True)
        pos = pos * rng.uniform(*scale)
        for axis, d in enumerate(degrees):
            pos = pos @ rotation(axis, math.radians(rng.uniform(-d, d)), pos.device).t()
        out.append(pos)
    return torch.cat(out, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dropout_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.data import MeshBatch
    from fieldconv_amd.dropout import tangent_dropout
    from fieldconv_amd.transforms import RandomMeshAffine
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), dtype='complex64', p=0.5, cases={})
    gen = torch.Generator().manual_seed(0)
    p, seed = 0.5, 2024

    for N, C in ((12500, 48), (20000, 64)):
        x = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
        gy = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev)
        step = torch.zeros(1, dtype=torch.int64, device=dev)

        def ours_fwd():
            with torch.no_grad():
                return tangent_dropout(x, p, seed, step)

        def comp_fwd():
            with torch.no_grad():
                return x * torch.nn.functional.dropout(torch.ones(N, C, device=dev), p)

        def ours_both():
            return torch.autograd.grad(tangent_dropout(x, p, seed, step), [x], gy)

        def comp_both():
            return torch.autograd.grad(x * torch.nn.functional.dropout(torch.ones(N, C, device=dev), p), [x], gy)
        y, y_ref = ours_fwd(), comp_fwd()
        case = dict(rows=N, channels=C, bytes_moved_per_pass=2 * 8 * N * C,
                    kept_fraction=dict(ours=float((y.real != 0).float().mean()), composite=float((y_ref.real != 0).float().mean())))
        case['forward'] = device_ms(ours_fwd, args.warmup, args.reps)
        case['forward_composite'] = device_ms(comp_fwd, args.warmup, args.reps)
        case['forward_backward'] = device_ms(ours_both, args.warmup, args.reps)
        case['forward_backward_composite'] = device_ms(comp_both, args.warmup, args.reps)
        case['forward_ratio'] = ratio(case['forward'], case['forward_composite'])
        case['forward_backward_ratio'] = ratio(case['forward_backward'], case['forward_backward_composite'])
        case['native_launches'] = dict(forward=1, backward=1)          # csrc/fc_dropout.hip; plus the clone of the device step forward
        res['cases'][f'dropout_{N}x{C}'] = case

    class Mesh:
        def __init__(self, pos):
            self.pos = pos
    B, V, scale, degrees = 8, 12500, (0.85, 1.15), (45.0, 45.0, 45.0)
    batch = MeshBatch.from_list([Mesh(torch.randn(V, 3, generator=gen)) for _ in range(B)]).to(dev)
    pos0 = batch.pos
    aug = RandomMeshAffine(scale=scale, degrees=degrees, center=True, seed=seed)
    rng = random.Random(0)

    def ours_aug():
        batch.pos = pos0
        return aug(batch).pos

    def loop_aug():
        batch.pos = pos0
        return loop_augment(batch, scale, degrees, rng)
    a, b = ours_aug(), loop_aug()
    batch.pos = pos0
    # the two draw different similarities: compare what a similarity about the centre preserves, the distances to the centre up to s
    ra = (a.view(B, V, 3).norm(dim=2) / (pos0.view(B, V, 3) - pos0.view(B, V, 3).mean(1, keepdim=True)).norm(dim=2))
    rb = (b.view(B, V, 3).norm(dim=2) / (pos0.view(B, V, 3) - pos0.view(B, V, 3).mean(1, keepdim=True)).norm(dim=2))
    case = dict(meshes=B, vertices_per_mesh=V, bytes_moved=2 * 12 * B * V,
                scale_spread_within_a_mesh=dict(ours=float((ra.max(1)[0] - ra.min(1)[0]).max()), loop=float((rb.max(1)[0] - rb.min(1)[0]).max())),
                scales=dict(ours=[round(float(v), 4) for v in ra.median(1)[0]], loop=[round(float(v), 4) for v in rb.median(1)[0]]))
    case['ours'] = device_ms(ours_aug, args.warmup, args.reps)
    case['loop'] = device_ms(loop_aug, args.warmup, args.reps)
    case['ratio'] = ratio(case['ours'], case['loop'])
    case['native_launches'] = dict(mean=2, draw=1, apply=1)
    res['cases'][f'augment_{B}x{V}'] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
