"""The walk kernels' record ring at every chunk event (csrc/fc_forward_ring.hpp, fc_backward_stream.hpp).

The ring-major forward kernel and the backward gather kernel read a vertex's records from a per-wavefront LDS ring of 1 KiB chunks
that arrive by LDS-DMA; inside the walk a chunk is not waited for -- that it has landed follows from the row values the walk has
used since the chunk's request (`ring_landed` in fc_forward_ring.hpp).  A record read before its chunk has landed would be a stale
or foreign record, so the mesh here is built by hand with the in-degree AND the out-degree of every vertex prescribed around every
chunk event: CR = records per chunk (8 / 16 factored records at band limit 3 / 2, 32 geometric ones), nr = chunks per ring (2 or 4):

    {0, 1, 2, 3, CR-2 .. CR+2, 2CR-2 .. 2CR+2, nr CR, nr CR + 1, 5 CR + 3}

spread over all sixteen rows of a tile (both streams of a forward wavefront), with ring runs that are random, a single run, or end
one before / exactly at / one behind a chunk boundary.  4 200 vertices: the smallest size that takes the ring-major forward kernel
(more than 256 tiles) and the H-streaming backward (at least 3 072 vertices).

Gates: the oracle at the suite's fp32 gate (max|d| <= 1e-5 max|ref|) for y, gx and the three parameter gradients; two runs bit for
bit; and the same bits, all finite, with NaNs right behind the records' documented padding (as tests/test_gpu_canary.py does)."""
import functools

import numpy as np
import pytest
import torch

N_VERTS = 4200
GATE = 1e-5
N_PATTERNS = 8
BIG_ROUNDS = 16          # a degree above CRmin + 2 goes to the first 16 vertices of its residue class only (every tile row once): the oracle's time


def chunk_records(B, geo):
    """(gather kernel, forward kernel): records per 1 KiB chunk -- factored records of round_up(4 + 2F, 4) floats, geometric ones of 8"""
    recf = (4 + 2 * (2 * B + 1) + 3) // 4 * 4
    per_kib = 256 // recf
    cr = 32 if per_kib >= 32 else 16 if per_kib >= 16 else 8 if per_kib >= 8 else 4
    return cr, (32 if geo else cr)


def degree_list(crs):
    deg = {0, 1, 2, 3}
    for cr in crs:
        deg |= set(range(cr - 2, cr + 3)) | set(range(2 * cr - 2, 2 * cr + 3)) | {5 * cr + 3}
        for nr in (2, 4):
            deg |= {nr * cr, nr * cr + 1}
    deg = sorted(deg)
    if len(deg) % 2 == 0:
        deg.append(5)          # an odd count: vertex v takes degree v % count, so every degree meets every row v % 16
    return deg


@functools.lru_cache(maxsize=None)
def build_mesh(R, B, geo, seed=0):
    """-> dict(edges (E,2) int64 sorted by source, sten (E,R,F) complex64, deg (N,), pattern (N,), q (E,), crs).

    Vertex v = i + k * len(degrees) has degree d = degrees[i] -- as a target and as a source -- and run pattern p = k % 8.  The
    vertices of one (d, p) class are joined among themselves: edge number s of member a runs to member a + 1 + s, where it is
    edge number s as well, so one ring index q(s) shapes the runs of both ends:
        p = 0  q random;   p = 1  one run;   p = 2 + 3 c + t  the first run ends at CR_c - 1 + t records, the rest is spread
        over the further runs in order."""
    F = 2 * B + 1
    crs = sorted(set(chunk_records(B, geo)))
    degrees = degree_list(crs)
    nd = len(degrees)
    big = min(crs) + 2
    rng = np.random.default_rng(seed)
    v = np.arange(N_VERTS)
    idx, k = v % nd, v // nd
    deg = np.asarray(degrees)[idx]
    deg[(deg > big) & (k >= BIG_ROUNDS)] = 2
    pattern = k % N_PATTERNS
    src, dst, q = [], [], []
    for d in np.unique(deg):
        if d == 0:
            continue
        for p in range(N_PATTERNS):
            members = np.flatnonzero((deg == d) & (pattern == p))
            m = len(members)
            if m == 0:
                continue
            s = np.arange(d)
            a = np.arange(m)
            if p == 0:
                qs = None
            elif p == 1:
                qs = np.full(d, (d + m) % (R - 1))
            else:
                cr = crs[((p - 2) // 3) % len(crs)]
                b = cr - 1 + (p - 2) % 3
                qs = np.where(s < b, 0, np.minimum(1 + ((s - b) * (R - 2)) // max(d - b, 1), R - 2))
            src.append(np.repeat(members, d))
            dst.append(members[(a[:, None] + 1 + s[None, :]) % m].reshape(-1))
            q.append(rng.integers(0, R - 1, size=m * d) if qs is None else np.tile(qs, m))
    src, dst, q = np.concatenate(src), np.concatenate(dst), np.concatenate(q)
    order = np.argsort(src, kind='stable')
    src, dst, q = src[order], dst[order], q[order]
    E = len(src)
    # FCPrecomp's shape of a stencil row: two adjacent rings, one phase vector -- geometric (c g^m, |g| = 1) or arbitrary
    w = rng.uniform(0.2, 1.0, size=(E, 2))
    if geo:
        ang = rng.uniform(0, 2 * np.pi, size=E)
        c = rng.uniform(0.2, 1.0, size=E) * np.exp(1j * rng.uniform(0, 2 * np.pi, size=E))
        ph = c[:, None] * np.exp(1j * ang[:, None] * np.arange(-B, B + 1)[None, :])
    else:
        ph = rng.standard_normal((E, F)) + 1j * rng.standard_normal((E, F))
    sten = np.zeros((E, R, F), dtype=np.complex64)
    rows = np.arange(E)
    sten[rows, q] = (w[:, 0:1] * ph * 0.2).astype(np.complex64)
    sten[rows, q + 1] = (w[:, 1:2] * ph * 0.2).astype(np.complex64)
    return dict(edges=np.stack((src, dst), 1).astype(np.int64), sten=sten, deg=deg, pattern=pattern, q=q, crs=crs, degrees=degrees)


CASES = [pytest.param(C, R, B, geo, id=f'C{C}-R{R}-B{B}-{"geometric" if geo else "factored"}')
         for C in (16, 48) for (R, B) in ((6, 2), (6, 3)) for geo in (True, False)]


@pytest.mark.parametrize('R,B,geo', [(6, 2, True), (6, 2, False), (6, 3, True), (6, 3, False)])
def test_mesh_has_every_degree_on_every_tile_row(R, B, geo):
    """(no GPU) the hand-built mesh is what the module's docstring says: every listed degree as in- and out-degree, on all sixteen tile
    rows; single runs; first runs that end at CR - 1, CR and CR + 1 records."""
    mesh = build_mesh(R, B, geo)
    src, dst, q, deg = mesh['edges'][:, 0], mesh['edges'][:, 1], mesh['q'], mesh['deg']
    assert np.array_equal(np.bincount(src, minlength=N_VERTS), deg)
    assert np.array_equal(np.bincount(dst, minlength=N_VERTS), deg)
    wanted = {0, 1, 2, 3}
    for cr in mesh['crs']:
        wanted |= set(range(cr - 2, cr + 3)) | set(range(2 * cr - 2, 2 * cr + 3)) | {2 * cr, 2 * cr + 1, 4 * cr, 4 * cr + 1, 5 * cr + 3}
    for d in sorted(wanted):
        rows = set((np.flatnonzero(deg == d) % 16).tolist())
        assert rows == set(range(16)), (d, sorted(rows))
    assert N_VERTS > 256 * 16 and N_VERTS >= 3072
    # run shapes, seen from the targets and from the sources
    for end in (dst, src):
        first = np.bincount(end[q == 0], minlength=N_VERTS)          # records of the first run
        nruns = np.zeros(N_VERTS, dtype=np.int64)
        for r in range(R - 1):
            nruns += np.bincount(end[q == r], minlength=N_VERTS) > 0
        one_run = (nruns == 1) & (deg > max(mesh['crs']))
        assert one_run.sum() >= 16                                   # all edges of a vertex in one run, several chunks long
        for cr in mesh['crs']:
            for b in (cr - 1, cr, cr + 1):
                assert ((first == b) & (deg > b)).sum() >= 16, (cr, b)


@functools.lru_cache(maxsize=None)
def reference(C, R, B, geo):
    """Inputs, parameters and the oracle's (y, gx, g_zonal, g_spherical, g_phase): computed once per case, never modified."""
    from oracle import fieldconv_oracle as orc
    from fieldconv_amd.nn import FieldConv
    mesh = build_mesh(R, B, geo)
    gen = torch.Generator().manual_seed(1000 * C + 10 * R + B)
    x = torch.complex(torch.randn(N_VERTS, C, generator=gen), torch.randn(N_VERTS, C, generator=gen))
    x[7] = 0
    gy = torch.complex(torch.randn(N_VERTS, C, generator=gen), torch.randn(N_VERTS, C, generator=gen))
    torch.manual_seed(C + R + B)
    conv = FieldConv(C, C, band_limit=B, n_rings=R, ftype=1)
    par = [p.detach().numpy().copy() for p in (conv.zonal, conv.spherical, conv.phase)]
    W = orc.effective_filter(par[0], par[1], par[2], 1, B)
    y, gx, gW = orc.fieldconv_forward_backward(x.numpy(), mesh['edges'], mesh['sten'], W, gy.numpy())
    gz, gs, gp = orc.effective_filter_vjp(gW, par[0], par[1], par[2], 1, B)
    return dict(x=x, gy=gy, state={k: v.clone() for k, v in conv.state_dict().items()}, ref=(y, gx, gz, gs, gp))


@pytest.mark.gpu
@pytest.mark.parametrize('C,R,B,geo', CASES)
def test_walk_kernels_at_every_chunk_event(C, R, B, geo):
    from fieldconv_amd.graph import SupportGraph
    from fieldconv_amd.nn import FieldConv
    dev = torch.device('cuda:0')
    mesh = build_mesh(R, B, geo)
    case = reference(C, R, B, geo)
    edges = torch.from_numpy(mesh['edges']).to(dev)
    sten = torch.from_numpy(mesh['sten']).to(dev)
    g = SupportGraph(edges, sten, N_VERTS)
    assert g.factored and (g.geo_t is not None) == geo          # the record-driven kernels, geometric records exactly where meant
    conv = FieldConv(C, C, band_limit=B, n_rings=R, ftype=1)
    conv.load_state_dict(case['state'])
    conv = conv.to(dev)
    x = case['x'].to(dev).requires_grad_(True)
    gy = case['gy'].to(dev)
    params = [conv.zonal, conv.spherical, conv.phase]

    def run():
        y = conv(x, edges, sten)
        grads = torch.autograd.grad(y, [x] + params, grad_outputs=gy)
        torch.cuda.synchronize()
        return [y.detach().clone()] + [t.clone() for t in grads]

    from fieldconv_amd.graph import register_graph
    register_graph(edges, sten, N_VERTS, g)
    first = run()
    names = ('y', 'gx', 'g_zonal', 'g_spherical', 'g_phase')
    errs = {}
    for name, got, ref in zip(names, first, case['ref']):
        got = got.cpu().numpy()
        errs[name] = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
    print('max|d| / max|ref| against the oracle:', errs)
    assert all(np.isfinite(v) and v <= GATE for v in errs.values()), errs

    second = run()
    for name, a, b in zip(names, first, second):
        assert torch.equal(a, b), f'{name}: two runs differ'

    # NaNs right behind the documented padding of the record arrays: an early or stray record read shows as a NaN
    originals = {}
    for name in ('rec_t', 'rec_s', 'geo_t'):
        t = getattr(g, name, None)
        if t is None:
            continue
        originals[name] = t
        buf = torch.empty(t.numel() * 4 + (1 << 20), dtype=torch.uint8, device=dev)
        buf[t.numel() * 4:].view(torch.float32).fill_(float('nan'))
        moved = buf[:t.numel() * 4].view(torch.float32).view(t.shape)
        moved.copy_(t)
        setattr(g, name, moved)
    g._plans.clear()
    try:
        third = run()
    finally:
        for name, t in originals.items():
            setattr(g, name, t)
        g._plans.clear()
    for name, a, b in zip(names, first, third):
        assert bool(torch.isfinite(torch.view_as_real(b) if b.is_complex() else b).all()), name
        assert torch.equal(a, b), f'{name}: differs with NaNs behind the record padding'
