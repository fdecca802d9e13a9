#!/usr/bin/env python3
"""What a mini-batch buys at the reference's operating point (not part of bench.py).

1. The config-3 network (tools/bench_net.py's topology and mesh recipe: 1 024 vertices, ~128 neighbours, 48 channels) on B = 8
   DIFFERENT meshes: (a) eight single-mesh forward + loss + backward steps with accumulated gradients -- the only way without
   MeshBatch, the baseline -- against (b) one step on the collated union with the per-mesh loss means through mesh_mean.
   Both are timed with the stencils already assembled (FCPrecomp's memo hits: the same tensors come back) and again with
   the collation and FCPrecomp inside the timed region.
2. farthest_point_sample_batched for 32 point sets of 10 000 points, 1 024 samples each, against 32 calls of
   farthest_point_sample.

Device events around each repetition, the variants alternating inside one process after a common warm-up; medians over
--reps repetitions.  Writes one JSON object (--out) and prints it.

    python tools/batch_throughput.py --out profiles/batch_throughput.json
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, start, stop):
    start.record()
    fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop)


def compare(variants, warmup, reps):
    """{name: [ms, ...]} with the variants alternating"""
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    out = {k: [] for k in variants}
    for _ in range(reps):
        for k, fn in variants.items():
            out[k].append(timed(fn, *ev))
    return out


def summary(ms):
    return dict(median_ms=round(statistics.median(ms), 4), min_ms=round(min(ms), 4), max_ms=round(max(ms), 4), reps=len(ms))


def net_case(args, dev):
    from fieldconv_amd.data import MeshBatch, sphere_support
    from fieldconv_amd.functional import mesh_mean
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock
    from fieldconv_amd.transforms import FCPrecomp
    N, k, nf, B, R, n_classes, nb = args.vertices, args.neighbours, 48, 2, 6, 8, args.meshes
    g = torch.Generator().manual_seed(0)
    meshes = []
    for i in range(nb):
        m = sphere_support(N, k, seed=i)
        m.pos, m.sample_idx = torch.randn(N, 3, generator=g), torch.arange(N)
        m.y = torch.randint(0, n_classes, (N,), generator=g)
        meshes.append(m.to(dev))
    eps = meshes[0].epsilon
    mods = torch.nn.ModuleDict(dict(
        lift=LiftBlock(3, nf, n_rings=R, ftype=1),
        r1=FCResNetBlock(nf, nf, band_limit=B, n_rings=R), r2=FCResNetBlock(nf, nf, band_limit=B, n_rings=R),
        r3=FCResNetBlock(nf, nf, band_limit=B, n_rings=R), r4=FCResNetBlock(nf, nf, band_limit=B, n_rings=R),
        echo=ECHOBlock(nf, n_classes, n_des=48, n_bins=3, band_limit=B, n_rings=R))).to(dev)
    params = list(mods.parameters())

    def logits_of(data, pre):
        edges, sten, ln, wxp = pre(data)
        x = mods['lift'](data.pos[data.sample_idx], edges, sten[..., B:B + 2])
        for name in ('r1', 'r2', 'r3', 'r4'):
            x = mods[name](x, edges, sten)
        return mods['echo'](x, edges, sten, ln, wxp)

    def accumulated(pres):
        for p in params:
            p.grad = None
        for m, pre in zip(meshes, pres):
            loss = torch.nn.functional.cross_entropy(logits_of(m, pre), m.y)
            (loss / nb).backward()

    def batched(batch, pre):
        for p in params:
            p.grad = None
        per_vertex = torch.nn.functional.cross_entropy(logits_of(batch, pre), batch.y, reduction='none')
        mesh_mean(per_vertex[:, None], batch.ptr).mean().backward()

    pres = [FCPrecomp(B, R, eps) for _ in meshes]
    union, union_pre = MeshBatch.from_list(meshes), FCPrecomp(B, R, eps)
    variants = {
        'accumulated_steps': lambda: accumulated(pres),
        'batched_step': lambda: batched(union, union_pre),
        'accumulated_steps_with_precomp': lambda: accumulated([FCPrecomp(B, R, eps) for _ in meshes]),
        'batched_step_with_collate_and_precomp': lambda: batched(MeshBatch.from_list(meshes), FCPrecomp(B, R, eps)),
    }
    # the two ways compute the same gradients
    accumulated(pres)
    ga = [p.grad.clone() for p in params]
    batched(union, union_pre)
    worst = max(float((p.grad - a).abs().max() / a.abs().max()) for p, a in zip(params, ga))
    ms = compare(variants, args.warmup, args.reps)
    res = {k: summary(v) for k, v in ms.items()}
    res.update(meshes=nb, vertices=N, neighbours=k, worst_gradient_rel_diff=worst,
               batched_over_accumulated=round(res['batched_step']['median_ms'] / res['accumulated_steps']['median_ms'], 4),
               batched_over_accumulated_with_precomp=round(res['batched_step_with_collate_and_precomp']['median_ms'] /
                                                           res['accumulated_steps_with_precomp']['median_ms'], 4))
    return res


def fps_case(args, dev):
    from fieldconv_amd.transforms import farthest_point_sample, farthest_point_sample_batched
    nb, n, S = args.fps_sets, args.fps_points, args.fps_samples
    g = torch.Generator().manual_seed(1)
    sets = [torch.rand(n, 3, generator=g).to(dev) for _ in range(nb)]
    pos = torch.cat(sets)
    ptr = torch.arange(nb + 1) * n
    same = torch.equal(farthest_point_sample_batched(pos, ptr, S), torch.cat([farthest_point_sample(p, S) for p in sets]))
    variants = {'single_calls': lambda: [farthest_point_sample(p, S) for p in sets],
                'batched_call': lambda: farthest_point_sample_batched(pos, ptr, S)}
    ms = compare(variants, max(2, args.warmup // 4), args.reps)
    res = {k: summary(v) for k, v in ms.items()}
    res.update(sets=nb, points=n, samples=S, identical_indices=same,
               speedup=round(res['single_calls']['median_ms'] / res['batched_call']['median_ms'], 2))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--meshes', type=int, default=8)
    ap.add_argument('--vertices', type=int, default=1024)
    ap.add_argument('--neighbours', type=int, default=128)
    ap.add_argument('--fps-sets', type=int, default=32)
    ap.add_argument('--fps-points', type=int, default=10000)
    ap.add_argument('--fps-samples', type=int, default=1024)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('batch_throughput.py measures on a ROCm device and none is visible')
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), net=net_case(args, dev), fps=fps_case(args, dev),
               launches_per_step='not measured (needs a kernel trace in a run of its own)')
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
