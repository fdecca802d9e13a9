#!/usr/bin/env python3
"""Generate tests/golden/mesh_batch.npz from the REFERENCE: what a mini-batch of four meshes must reproduce.

The reference trains with batch_size = 1 and emulates a batch by gradient accumulation (`L = L / batch_step; L.backward()` in
its notebooks' train()).  This script does exactly that with the reference's own modules, one mesh at a time, for four
synthetic meshes of different sizes and two network topologies, and stores the per-mesh logits, the per-mesh losses and the
ACCUMULATED parameter gradients -- the numbers one batched step on the collated union has to match:

    classification   LiftBlock(3 -> C), two FCResNetBlocks, FieldConv(C -> classes), mean(softAbs(x), dim=0) + bias, cross-entropy
                     against one label per mesh (the topology of the reference's classification.ipynb Net)
    segmentation     LiftBlock(3 -> C), two FCResNetBlocks, ECHOBlock(C -> classes), log-softmax NLL against per-vertex labels

It imports the reference through make_golden.py (reference `nn`, `transforms/fc_precomp.py`, behind tests/golden/_refstubs),
reuses its synthetic log-map recipe, fills the parameters from param_fill.py, and stores data only.  Yardsticks, measured with
the reference itself as make_golden.py's correspondence case does: every tensor again with the input positions perturbed by
a few ulp (relative 3e-7, eight twins, the largest deviation kept: cond_* / gcond_<name>), and the classification net again in
float64 (the reference's ECHO is float32-only, so the segmentation net has no float64 run).

    python tests/golden/make_golden_batch.py            # rewrites tests/golden/mesh_batch.npz
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import _Data, np_, ref_fc_precomp, refnn, synthetic_logmap          # noqa: E402  (imports the reference)
from param_fill import fill_params                                                  # noqa: E402

SIZES = (40, 97, 64, 150)
K, B, R, EPS = 7, 2, 6, 0.2
C, N_CLASSES, N_DES, N_BINS = 8, 4, 6, 2
N_TWINS = 8


class ClassificationNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        kw = dict(band_limit=B, n_rings=R, ftype=1)
        self.lift = refnn.LiftBlock(3, C, n_rings=R, ftype=1)
        self.resnet1 = refnn.FCResNetBlock(C, C, **kw)
        self.resnet2 = refnn.FCResNetBlock(C, C, **kw)
        self.conv_out = refnn.FieldConv(C, N_CLASSES, **kw)
        self.bias = torch.nn.Parameter(torch.zeros(1, N_CLASSES))

    def forward(self, pos, edges, sten, ln, wxp):
        from utils.field import softAbs          # the reference's
        x = self.lift(pos, edges, sten[..., B:B + 2])
        x = self.resnet2(self.resnet1(x, edges, sten), edges, sten)
        x = self.conv_out(x, edges, sten)
        return torch.mean(softAbs(x), dim=0, keepdim=True) + self.bias


class SegmentationNet(torch.nn.Module):
    def __init__(self):
        super().__init__()
        kw = dict(band_limit=B, n_rings=R, ftype=1)
        self.lift = refnn.LiftBlock(3, C, n_rings=R, ftype=1)
        self.resnet1 = refnn.FCResNetBlock(C, C, **kw)
        self.resnet2 = refnn.FCResNetBlock(C, C, **kw)
        self.echo = refnn.ECHOBlock(C, N_CLASSES, n_des=N_DES, n_bins=N_BINS, **kw)

    def forward(self, pos, edges, sten, ln, wxp):
        x = self.lift(pos, edges, sten[..., B:B + 2])
        x = self.resnet2(self.resnet1(x, edges, sten), edges, sten)
        return self.echo(x, edges, sten, ln, wxp)


def accumulate(net, meshes, positions, labels, dtype=torch.float32):
    """The reference's batching: one mesh per step, L / batch_step, gradients summed by autograd.
    -> per-mesh logits, per-mesh losses, {name: accumulated gradient}"""
    net.zero_grad()
    logits, losses = [], []
    for (edges, sten, ln, wxp), pos, y in zip(meshes, positions, labels):
        if dtype == torch.float64:
            sten = sten.to(torch.cdouble)
        out = net(pos.to(dtype), edges, sten, ln, wxp)
        L = torch.nn.functional.cross_entropy(out, y)
        (L / len(meshes)).backward()
        logits.append(out.detach().clone())
        losses.append(L.detach().clone())
    return logits, torch.stack(losses), {n: p.grad.detach().clone() for n, p in net.named_parameters()}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max())


def net_case(out, tag, net, meshes, positions, labels, with_f64):
    fill_params(net)
    logits, losses, grads = accumulate(net, meshes, positions, labels)
    cond_logits, cond_loss, gcond = 0.0, 0.0, {n: 0.0 for n in grads}
    for twin in range(N_TWINS):
        gp = torch.Generator().manual_seed(99 + twin)
        pert = [p * (1 + 3e-7 * (2 * torch.rand(p.shape, generator=gp) - 1)) for p in positions]
        lg_p, ls_p, gr_p = accumulate(net, meshes, pert, labels)
        cond_logits = max(cond_logits, rel(torch.cat(lg_p), torch.cat(logits)))
        cond_loss = max(cond_loss, float((ls_p - losses).abs().max() / losses.abs().max()))
        gcond = {n: max(gcond[n], rel(gr_p[n], grads[n])) for n in grads}
    rec = dict(logits=np_(torch.cat(logits)), losses=np_(losses), cond_logits=cond_logits, cond_loss=cond_loss, n_twins=N_TWINS,
               n_params=sum(p.numel() for p in net.parameters()))
    for n in grads:
        rec['g_' + n] = np_(grads[n])
        rec['gcond_' + n] = gcond[n]
    if with_f64:
        lg64, ls64, gr64 = accumulate(net.double(), meshes, positions, labels, dtype=torch.float64)
        rec['logits64'], rec['losses64'] = np_(torch.cat(lg64)), np_(ls64)
        for n in gr64:
            rec['g64_' + n] = np_(gr64[n])
    out[tag] = rec


def main():
    out = {}
    meshes, positions, raw = [], [], {}
    for i, N in enumerate(SIZES):
        g = torch.Generator().manual_seed(5150 + i)
        edges, logMag, logAng, xp, w = synthetic_logmap(g, N, K, EPS)
        d = _Data()
        d.logMag, d.logAng, d.w, d.supp_edges, d.xp = logMag, logAng, w, edges, xp
        meshes.append(ref_fc_precomp.FCPrecomp(B, R, EPS)(d))
        pos = torch.randn(N, 3, generator=g)
        positions.append(pos)
        raw.update({f'edges_{i}': np_(edges), f'logMag_{i}': np_(logMag), f'logAng_{i}': np_(logAng), f'xp_{i}': np_(xp), f'w_{i}': np_(w),
                    f'pos_{i}': np_(pos), f'kept_edges_{i}': meshes[-1][0].shape[0]})
    g = torch.Generator().manual_seed(6006)
    y_mesh = [torch.randint(0, N_CLASSES, (1,), generator=g) for _ in SIZES]
    y_vertex = [torch.randint(0, N_CLASSES, (N,), generator=g) for N in SIZES]
    raw.update(dict(sizes=np.array(SIZES), B=B, R=R, eps=EPS, C=C, n_classes=N_CLASSES, n_des=N_DES, n_bins=N_BINS,
                    y_mesh=np_(torch.cat(y_mesh)), y_vertex=np_(torch.cat(y_vertex))))
    out['meshes'] = raw
    torch.manual_seed(0)
    net_case(out, 'classification', ClassificationNet(), meshes, positions, y_mesh, with_f64=True)
    net_case(out, 'segmentation', SegmentationNet(), meshes, positions, y_vertex, with_f64=False)
    flat = {f'{tag}/{key}': np.asarray(val) for tag, rec in out.items() for key, val in rec.items()}
    path = os.path.join(HERE, 'mesh_batch.npz')
    np.savez_compressed(path, **flat)
    print(f'mesh_batch.npz: {len(out)} cases, {os.path.getsize(path) / 1024:.0f} KiB')
    for tag in ('classification', 'segmentation'):
        r = out[tag]
        print(tag, 'cond_logits %.1e cond_loss %.1e worst gcond %.1e' % (r['cond_logits'], r['cond_loss'],
                                                                         max(v for k, v in r.items() if k.startswith('gcond_'))))


if __name__ == '__main__':
    main()
