#!/usr/bin/env python3
"""TangentNorm (fieldconv_amd.norm, csrc/fc_norm.hip) beside the stock-op composite on the same device (not part of bench.py).

    cases       complex64, C = 48: 8 meshes of 1 024 rows with integration weights w; one mesh of 20 000 rows without
    passes      forward, and forward + backward (gradients to x and gain)
    composite   per mesh: index_add_ of w |x|^2 and of w, a division, rsqrt, a gather of the scale by the row's mesh, a multiply;
                autograd for its backward

Device events around each repetition after a common warm-up, median of --reps (5): the protocol of tools/geodesic_throughput.py.
Writes one JSON object (--out).  Nothing is gated; box-to-box noise is +-5 %.

    python tools/norm_throughput.py --out profiles/norm_throughput.json
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


def composite(x, gain, mesh_of_row, B, w, eps):
    """the layer from stock ops: (N,C) temporaries each way, atomics in index_add_"""
    wn = torch.ones(x.shape[0], dtype=x.real.dtype, device=x.device) if w is None else w.reshape(-1)
    s = torch.zeros(B, x.shape[1], dtype=wn.dtype, device=x.device).index_add_(0, mesh_of_row, wn[:, None] * x.abs().pow(2))
    W = torch.zeros(B, dtype=wn.dtype, device=x.device).index_add_(0, mesh_of_row, wn)
    m = torch.where(W[:, None] > 0, s / W[:, None].clamp_min(torch.finfo(wn.dtype).tiny), torch.zeros_like(s))
    return (gain * torch.rsqrt(m + eps))[mesh_of_row] * x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('norm_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.norm import tangent_norm
    from fieldconv_amd.pooling import tag_ptr
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), dtype='complex64', channels=48, cases={})
    C, eps = 48, 1e-5
    gen = torch.Generator().manual_seed(0)

    for name, counts, weighted in (('8x1024_w', [1024] * 8, True), ('1x20000', [20000], False)):
        host = [0]
        for n in counts:
            host.append(host[-1] + n)
        N, B = host[-1], len(counts)
        ptr = tag_ptr(torch.tensor(host, dtype=torch.int64).to(dev), host)
        mesh_of_row = torch.repeat_interleave(torch.arange(B, device=dev), torch.tensor(counts, device=dev))
        x = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev).requires_grad_(True)
        gy = torch.complex(torch.randn(N, C, generator=gen), torch.randn(N, C, generator=gen)).to(dev)
        gain = (0.5 + torch.rand(1, C, generator=gen)).to(dev).requires_grad_(True)
        w = (0.1 + 2 * torch.rand(N, generator=gen)).to(dev) if weighted else None

        def ours_fwd():
            with torch.no_grad():
                return tangent_norm(x, gain, ptr, w, eps)

        def comp_fwd():
            with torch.no_grad():
                return composite(x, gain, mesh_of_row, B, w, eps)

        def ours_both():
            return torch.autograd.grad(tangent_norm(x, gain, ptr, w, eps), [x, gain], gy)

        def comp_both():
            return torch.autograd.grad(composite(x, gain, mesh_of_row, B, w, eps), [x, gain], gy)
        y, y_ref = ours_fwd(), comp_fwd()
        (gx, gg), (gx_ref, gg_ref) = ours_both(), comp_both()
        case = dict(rows=N, meshes=B, weights=weighted,
                    max_abs_difference_from_composite=dict(y=float((y - y_ref).abs().max()), gx=float((gx - gx_ref).abs().max()),
                                                           ggain=float((gg - gg_ref).abs().max())),
                    largest_entry=dict(y=float(y_ref.abs().max()), gx=float(gx_ref.abs().max()), ggain=float(gg_ref.abs().max())))
        case['forward'] = device_ms(ours_fwd, args.warmup, args.reps)
        case['forward_composite'] = device_ms(comp_fwd, args.warmup, args.reps)
        case['forward_backward'] = device_ms(ours_both, args.warmup, args.reps)
        case['forward_backward_composite'] = device_ms(comp_both, args.warmup, args.reps)
        case['forward_ratio'] = ratio(case['forward'], case['forward_composite'])
        case['forward_backward_ratio'] = ratio(case['forward_backward'], case['forward_backward_composite'])
        case['native_launches'] = dict(forward=3, backward=4)          # csrc/fc_norm.hip; the composite's are torch's own and not counted
        res['cases'][name] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
