"""What the explicit vector-memory waits of the two walk kernels cost (development).

    python tools/wait_cost.py [--shape N k C B R] [--out FILE]

Runs the layer a few times, then one step with the stamp buffer armed and FC_STAMP_KERNEL=waits: every wavefront of the ring-major
forward kernel and of the backward gather kernel sums the shader cycles it stands in each kind of `s_waitcnt` (WaitMeter,
csrc/fc_common.hpp).  Prints, per kind: waits per launch, cycles per wait, and the waits' share of the wavefronts' own cycles -- an
upper bound of the share of the launch, since a SIMD's other wavefronts issue while one waits."""
import argparse
import ctypes
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__  # noqa: E402

KINDS = {
    'forward ring kernel': (0, {0: 'chunk entry', 1: 'look-ahead at CR-2 (nr = 2)', 2: 'targets done, before the next chunks',
                                3: "next tile's first chunks", 4: 'first chunks (prologue)', 7: '(two clock reads around nothing)'}),
    'backward gather kernel': (32, {0: 'chunk entry', 1: 'walk done, before the next chunks', 2: 'first chunks (walk start)',
                                    7: '(two clock reads around nothing)'}),
}


def table(buf):
    lines = []
    for name, (base, kinds) in KINDS.items():
        s = buf[base:base + 32].tolist()
        total, waves = s[16], s[17]
        lines.append(f'{name}: {waves} wavefronts, {total} wavefront cycles ({total // max(waves, 1)} per wavefront)')
        lines.append(f'  {"wait":42s} {"per launch":>11s} {"cycles/wait":>12s} {"cycles":>12s} {"share":>7s}')
        null = s[7] / s[15] if s[15] else 0.0
        for k, label in kinds.items():
            cyc, n = s[k], s[8 + k]
            lines.append(f'  {label:42s} {n:11d} {cyc / n if n else 0.0:12.1f} {cyc:12d} {100.0 * cyc / total if total else 0.0:6.2f}%')
        net = sum(s[k] - null * s[8 + k] for k in kinds if k != 7)
        lines.append(f'  all waits, the clock reads taken off: {100.0 * net / total if total else 0.0:.2f}% of the wavefront cycles')
    return '\n'.join(lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shape', type=int, nargs=5, default=[20000, 32, 48, 2, 6], metavar=('N', 'k', 'C', 'B', 'R'))
    ap.add_argument('--warm', type=int, default=200, help='steps before the metered one (the settled clock)')
    ap.add_argument('--out', default=None, help='also write the table to this file')
    args = ap.parse_args()
    os.environ['FC_STAMP_KERNEL'] = 'waits'
    if not os.environ.get('FIELDCONV_HIP_LIB'):
        from fieldconv_amd import build as _b
        if _b.needs_build() or _b.dev_needs_build():
            __graft_entry__.build()
        os.environ['FIELDCONV_HIP_LIB'] = _b.DEV_LIB_PATH     # the meter exists in the development build only
    from fieldconv_amd import _lib
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.nn import FieldConv
    from fieldconv_amd.transforms import FCPrecomp
    dev = torch.device('cuda:0')
    N, k, C, B, R = args.shape
    data = sphere_support(N, k, support='p95').to(dev)
    edges, sten, _, _ = FCPrecomp(B, R, data.epsilon)(data)
    conv = FieldConv(C, C, band_limit=B, n_rings=R).to(dev)
    x = torch.randn(N, C, dtype=torch.cfloat, device=dev).requires_grad_(True)
    gy = torch.randn(N, C, dtype=torch.cfloat, device=dev)
    params = list(conv.parameters())

    def step():
        y = conv(x, edges, sten)
        torch.autograd.grad(y, [x] + params, grad_outputs=gy)
    for _ in range(args.warm):
        step()
    torch.cuda.synchronize()
    buf = torch.zeros(16 * 256, dtype=torch.int64, device=dev)
    lib = _lib.load()
    lib.fc_debug_stamp_buffer(ctypes.c_void_p(buf.data_ptr()))
    step()
    torch.cuda.synchronize()
    lib.fc_debug_stamp_buffer(None)
    text = f'shape N={N} k={k} C={C} B={B} R={R}, library {os.path.basename(os.environ["FIELDCONV_HIP_LIB"])}\n' + table(buf.cpu())
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
