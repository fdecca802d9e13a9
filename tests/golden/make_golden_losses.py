#!/usr/bin/env python3
"""Generate tests/golden/losses.npz from the REFERENCE's TwinLoss, TwinEval and LabelSmoothingLoss.

Runs only where a checkout of the reference is: FIELDCONV_REFERENCE names its directory.  The three modules are imported
unmodified by file path and run on the CPU with seeded inputs; inputs, the random weights TwinLoss drew (recovered by
reseeding torch's CPU generator and redrawing), outputs and autograd gradients are stored.  Data only: no reference source
is copied.  The reference's TwinLoss accumulates into a float32 tensor, so its loss is float32 whatever the features' dtype;
it is stored as returned.

    FIELDCONV_REFERENCE=... python tests/golden/make_golden_losses.py            # rewrites tests/golden/losses.npz
"""
import importlib.util
import os

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get('FIELDCONV_REFERENCE')
if not REF:
    raise SystemExit('set FIELDCONV_REFERENCE to the directory of the reference checkout')


def _load(name):
    spec = importlib.util.spec_from_file_location('ref_' + name, os.path.join(REF, 'nn', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TwinLoss = _load('twin_loss').TwinLoss
TwinEval = _load('twin_eval').TwinEval
LabelSmoothingLoss = _load('label_smoothing_loss').LabelSmoothingLoss


def np_(t):
    return t.detach().cpu().numpy()


def twin_cases(out):
    """Inputs are float32 values, stored once per case; the float64 run uses the same values widened."""
    C = 16
    for name, N, P, M, repeated in (('n300', 300, 200, 256, False), ('repeat', 60, 180, 220, True)):
        g = torch.Generator().manual_seed(11 if repeated else 7)
        # spread so that mu - d2 takes both signs over the negatives
        xS0 = torch.rand(N, C, generator=g) * 0.9
        xT0 = torch.rand(N, C, generator=g) * 0.9
        if repeated:
            # every pair hits row 5 of xT; xS rows come from a handful, many times each
            p_ = torch.stack((torch.full((P,), 5), torch.randint(0, 4, (P,), generator=g)), 1)
            n_ = torch.stack((torch.full((M,), 5), torch.randint(0, 7, (M,), generator=g) * 8), 1)
        else:
            p_ = torch.stack((torch.randperm(N, generator=g)[:P], torch.randint(0, N, (P,), generator=g)), 1)
            n_ = torch.randint(0, N, (M, 2), generator=g)
        mu = 2.5
        key = f'twin_{name}'
        out.update({f'{key}/xS': np_(xS0), f'{key}/xT': np_(xT0), f'{key}/p': np_(p_), f'{key}/n': np_(n_), f'{key}/mu': np.float64(mu),
                    f'{key}/eval_ratio': np.float64(0.9)})
        for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
            xS = xS0.to(dt).requires_grad_(True)
            xT = xT0.to(dt).requires_grad_(True)
            torch.manual_seed(123)
            loss = TwinLoss(mu=mu)(xS, xT, p_, n_)
            torch.manual_seed(123)
            yN = 0.2 * torch.rand(M).float()
            gS, gT = torch.autograd.grad(loss, [xS, xT])
            nFN, nFP = TwinEval(mu=mu, ratio=0.9)(xS.detach(), xT.detach(), p_, n_)
            out.update({f'{key}/yN': np_(yN), f'{key}/loss_{tag}': np_(loss), f'{key}/gS_{tag}': np_(gS), f'{key}/gT_{tag}': np_(gT),
                        f'{key}/nFN_{tag}': np.int64(nFN), f'{key}/nFP_{tag}': np.int64(nFP)})


def smoothing_cases(out):
    """Per shape: float32 inputs stored once; variants (smoothing, weighted) in float32, and the smoothing 0.1 weighted one in
    float64 too (the same values widened).  classes != K at (257, 40) with smoothing 0.1 and weights."""
    for (N, K) in ((1024, 8), (1, 30), (257, 40)):
        g = torch.Generator().manual_seed(1000 * K + N)
        pred0 = 2.0 * torch.randn(N, K, generator=g)
        target = torch.randint(0, K, (N,), generator=g)
        weight0 = 0.5 + torch.rand(K, generator=g)
        key = f'ls_{N}x{K}'
        out.update({f'{key}/pred': np_(pred0), f'{key}/target': np_(target), f'{key}/weight': np_(weight0)})
        variants = [(0.0, False), (0.1, False), (0.1, True)] + ([(0.0, True)] if N == 1 else [])
        names = []
        for smoothing, weighted in variants:
            classes = K + 3 if (N, smoothing, weighted) == (257, 0.1, True) else K
            for dt, tag in ((torch.float32, 'f32'), (torch.float64, 'f64')):
                if tag == 'f64' and not (smoothing == 0.1 and weighted):
                    continue
                pred = pred0.to(dt).requires_grad_(True)
                weight = weight0.to(dt) if weighted else None
                loss = LabelSmoothingLoss(classes, smoothing=smoothing, dim=1, weight=weight)(pred, target)
                gp, = torch.autograd.grad(loss, [pred])
                v = f's{int(round(smoothing * 10))}_{"w" if weighted else "u"}_c{classes}_{tag}'
                names.append(v)
                out.update({f'{key}/loss_{v}': np_(loss), f'{key}/gpred_{v}': np_(gp)})
        out[f'{key}/variants'] = np.array(names)


def main():
    out = {}
    twin_cases(out)
    smoothing_cases(out)
    path = os.path.join(HERE, 'losses.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes,', len(out), 'arrays')


if __name__ == '__main__':
    main()
