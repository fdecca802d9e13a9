#!/usr/bin/env python3
"""FusedAdam's controls (fc_adam_step_ctl: device learning rate, global-norm clipping, non-finite skip, decoupled weight decay, moving
average) beside the plain FusedAdam step and beside stock torch on the same device (not part of bench.py).

On the parameter set of the config-3 network (tools/bench_net.py: LiftBlock(3->48), four FCResNetBlocks, ECHOBlock(48->8)):

    bare        opt.step() on gradients that already lie in the flat buffer: every control on (3 launches) against the plain step
                (2 launches, the code from before the controls) in the same run
    torch       the same against torch.nn.utils.clip_grad_norm_(foreach=True) + torch.optim.AdamW(foreach=True).step()
    replayed    the whole training step (forward, loss, backward, step) of the network on a 1024-vertex sphere as one StepGraph, with and
                without the controls

Device events around each repetition after a common warm-up, median of --reps (5), min and max kept: the protocol of
tools/geodesic_throughput.py; a repetition of the bare cases is --inner (20) calls, reported per call.  Writes one JSON object
(--out).  Nothing is gated; box-to-box noise is +-5 %.

    python tools/optim_controls_throughput.py --out profiles/optim_controls_throughput.json
"""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from geodesic_throughput import device_ms, ratio          # noqa: E402  (the same protocol)

CONTROLS = dict(decoupled_weight_decay=True, max_grad_norm=1.0, skip_nonfinite=True, ema_decay=0.999, device_lr=True)
N, K, NF, B, R, N_CLASSES = 1024, 128, 48, 2, 6, 8


def network():
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock
    torch.manual_seed(0)
    return torch.nn.ModuleDict(dict(
        lift=LiftBlock(3, NF, n_rings=R, ftype=1),
        r1=FCResNetBlock(NF, NF, band_limit=B, n_rings=R), r2=FCResNetBlock(NF, NF, band_limit=B, n_rings=R),
        r3=FCResNetBlock(NF, NF, band_limit=B, n_rings=R), r4=FCResNetBlock(NF, NF, band_limit=B, n_rings=R),
        echo=ECHOBlock(NF, N_CLASSES, n_des=48, n_bins=3, band_limit=B, n_rings=R)))


def per_call(fn, inner, warmup, reps):
    def many():
        for _ in range(inner):
            fn()
    t = device_ms(many, warmup, reps)
    return dict(median_ms=round(t['median_ms'] / inner, 5), min_ms=round(t['min_ms'] / inner, 5), max_ms=round(t['max_ms'] / inner, 5),
                reps=reps, calls_per_rep=inner)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--inner', type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('optim_controls_throughput.py measures on a ROCm device and none is visible')
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.optim import FusedAdam
    from fieldconv_amd.transforms import FCPrecomp
    from fieldconv_amd.utils import StepGraph
    dev = torch.device('cuda:0')
    res = dict(device=torch.cuda.get_device_name(0), controls={k: v for k, v in CONTROLS.items()}, cases={})
    kw = dict(lr=1e-3, weight_decay=1e-2)
    gen = torch.Generator().manual_seed(0)

    # ---- the bare optimizer call on the network's parameter set
    nets = [network().to(dev) for _ in range(3)]
    plain = FusedAdam(nets[0].parameters(), **kw)
    ctl = FusedAdam(nets[1].parameters(), **kw, **CONTROLS)
    grad = (torch.randn(plain._n, generator=gen) * 1e-2).to(dev)
    plain._grad.copy_(grad)
    ctl._grad.copy_(grad)
    stock_params = list(nets[2].parameters())
    for p, o, n in zip(stock_params, plain._offsets, plain._sizes):
        p.grad = grad[o:o + n].view(p.shape).clone()
    stock = torch.optim.AdamW(stock_params, foreach=True, **kw)

    def stock_step():
        torch.nn.utils.clip_grad_norm_(stock_params, CONTROLS['max_grad_norm'], foreach=True)
        stock.step()
    case = dict(parameter_tensors=len(plain._sizes), floats=plain._n, native_launches=dict(plain=2, controls=3))
    case['plain'] = per_call(plain.step, args.inner, args.warmup, args.reps)
    case['controls'] = per_call(ctl.step, args.inner, args.warmup, args.reps)
    case['torch_clip_adamw'] = per_call(stock_step, args.inner, args.warmup, args.reps)
    case['controls_over_plain'] = ratio(case['controls'], case['plain'])
    case['controls_over_torch'] = ratio(case['controls'], case['torch_clip_adamw'])
    case['skipped_steps'] = float(ctl.skipped()[1])
    res['cases']['bare_step'] = case

    # ---- the whole training step, replayed
    data = sphere_support(N, K).to(dev)
    pre = FCPrecomp(B, R, data.epsilon)
    pos = torch.randn(N, 3, generator=gen).to(dev)
    labels = torch.randint(0, N_CLASSES, (N,), generator=gen).to(dev)

    def step_of(mods, opt):
        def step():
            edges, sten, ln, wxp = pre(data)
            x = mods['lift'](pos, edges, sten[..., B:B + 2])
            for name in ('r1', 'r2', 'r3', 'r4'):
                x = mods[name](x, edges, sten)
            logits = mods['echo'](x, edges, sten, ln, wxp)
            loss = torch.nn.functional.nll_loss(torch.nn.functional.log_softmax(logits, dim=1), labels)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()
        return step
    case = dict(vertices=N, neighbours=K)
    for label, extra in (('plain', {}), ('controls', CONTROLS)):
        mods = copy.deepcopy(nets[2])
        opt = FusedAdam(mods.parameters(), **kw, **extra)
        graphed = StepGraph(step_of(mods, opt))
        case[label] = device_ms(graphed.replay, args.warmup, args.reps)
    case['controls_over_plain'] = ratio(case['controls'], case['plain'])
    res['cases']['replayed_step'] = case

    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
