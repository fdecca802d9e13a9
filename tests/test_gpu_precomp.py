"""FCPrecomp and the support-graph build (csrc/fc_precomp.hip, csrc/fc_graph.hip) EDGE BY EDGE on planted supports (inputs and the
float64 / structural restatements: _precomp_cases.py, pinned on the CPU by test_precomp_host.py).

Exact: the kept edges and their dtype, the ring index of every edge (decided by the same float32 arithmetic on both sides: radii sit
on the knots, at 0, at epsilon and one ulp to either side), rowptr / perm / nbr / runs of both sides against a stable sort by
(vertex, ring, edge id), the slot-order records against the edge-order ones bit for bit, every padding row, every exact zero, and ln
between the fused and the literal build.  Per edge, over the edge's OWN scale (|wxp_e| for rows, phases and c, max(r, 1e-30) for ln, 1
for the weights and g): gate = 4 x the float32 restatement's per-edge error against the float64 one on the same case, floor 1e-6,
computed at run time from the CPU restatements, never from the device result.

Rows built from powers of g = e^{i theta} (the factor table: FactoredStencil.materialize, geo_t) are compared with the restatement
that forms m * theta in float64, rows built from sin / cos of the float32 product (the literal builder, rec_t / rec_s) with the one
that forms it in float32, as the reference does (_precomp_cases.py has the bound between the two).

B = 0 has no record-driven kernels (fc_shape_compiled), so FCPrecomp hands back the literal rows for `B0-R6` like for the `literal-*`
cases; its records (F = 1, 8 floats) are checked through fc_graph_build instead (test_graph_build_from_dense_stencil).

Largest device error / its gate over all cases and two runs (MI355X); nearly every maximum is many-long-runs (in-degree 109; the area sums
are float atomics, so wxp moves from run to run), whose float32 restatement is itself 5e-7 .. 1e-6 off; every other case stays below
3.3e-7 under gates of 1.0e-6 .. 2.6e-6:
    fused        ln 1.00e-07 / 1.00e-06   wxp = c 5.78e-07 / 2.16e-06   w0 4.47e-08 / 2.16e-06   w1 2.98e-08 / 2.04e-06   g 7.75e-08 / 1.00e-06
                 phases of rec_t 6.33e-07 / 3.96e-06   materialised rows 6.15e-07 / 3.96e-06
    literal      rows 5.24e-07 / 3.96e-06   ln 1.00e-07 / 1.00e-06   wxp 5.96e-07 / 2.16e-06
    graph build  w0 2.16e-07   w1 1.82e-07   phases 1.17e-07 (knots-R3-e1)   c 1.16e-07   g 2.17e-07, all / 1.00e-06
                 (R = 2, knots-R2-e1 / -e03: w0 1.31e-07   w1 1.20e-07   phases 1.11e-07   c 1.08e-07   g 1.72e-07)
    row scaling  rows from the records: native 2.52e-07, torch 2.34e-07 / 2.43e-06; convolution row-wise 4.64e-07 / 1.00e-05
The gates move a little with the CPU: the float32 restatement's knots are torch.sqrt's, which is not correctly rounded everywhere."""
import os

import numpy as np
import pytest
import torch

import _precomp_cases as pc
from _dynamic_range_cases import measured_err
from oracle import fieldconv_oracle as orc

pytestmark = pytest.mark.gpu
REDUCED = os.environ.get('FC_MFMA') == 'f16'
CONV_TOL = 5e-3 if REDUCED else 1e-5         # the row-wise gate of y in test_gpu_dynamic_range.py

FUSED_CASES = [n for n in pc.CASES if n not in pc.DENSE_CASES and n != 'none-kept']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def device_data(name, dev):
    """the case on the device; `dups-i32` hands the edges over as int32, `dups-T` as the transposed view of a (2,E) tensor"""
    data = pc.support_data(name).to(dev)
    if name == 'dups-i32':
        data.supp_edges = data.supp_edges.to(torch.int32)
    if name == 'dups-T':
        data.supp_edges = data.supp_edges.t().contiguous().t()
        assert not data.supp_edges.is_contiguous()
    return data


def run(name, dev, monkeypatch, literal):
    from fieldconv_amd.transforms import FCPrecomp
    B, R, eps = pc.CASES[name]
    for var in ('FIELDCONV_EAGER_STENCIL', 'FIELDCONV_DENSE', 'FIELDCONV_NO_GEO'):
        monkeypatch.delenv(var, raising=False)
    if literal:
        monkeypatch.setenv('FIELDCONV_EAGER_STENCIL', '1')
    data = device_data(name, dev)
    out = FCPrecomp(B, R, eps)(data)
    assert out[0].dtype == data.supp_edges.dtype and out[0].device == data.supp_edges.device
    return out


def check(label, got, own):
    """the device's per-edge errors `got` within the gates that the float32 restatement's errors `own` give; prints all three"""
    parts, bad = [], []
    for key, err in got.items():
        gate = pc.gate_of(own[key])
        parts.append('%s %.2e (own %.2e, gate %.2e)' % (key, err, own[key], gate))
        if not err <= gate:
            bad.append(key)
    print('\n%s: %s' % (label, '  '.join(parts)))
    assert not bad, (label, bad)


def check_dense_rows(name, sten, key):
    """a dense (E',R,F) stencil of the device against the restatement `key`: entries the restatement has as exact zeros are exact
    zeros, entries it has above the float32 denormals are not -- every ring of every row, no magnitude mask"""
    ref = pc.precomp_ref(name)[key]
    assert sten.shape == ref.shape and sten.dtype == np.complex64
    assert not sten[ref == 0].any()
    assert (sten[np.abs(ref) >= 2.0 ** -125] != 0).all()


def check_literal(name, out):
    ref = pc.precomp_ref(name)
    edges, sten, ln, wxp = out
    assert torch.is_tensor(sten) and sten.dtype == torch.complex64 and sten.is_contiguous()
    assert np.array_equal(H(edges).astype(np.int64), ref['edges'])
    check_dense_rows(name, H(sten), 'sten')
    check('literal %s' % name, pc.errors(name, dict(sten=H(sten), ln=H(ln), wxp=H(wxp))), pc.own_errors(name))


# ---------------------------------------------------------------------------------------------- 1. the fused path
@pytest.mark.parametrize('name', FUSED_CASES)
def test_fused_path(name, dev, monkeypatch):
    from fieldconv_amd.graph import FactoredStencil, get_graph
    B, R, eps = pc.CASES[name]
    F, N = 2 * B + 1, pc.case(name)['N']
    ref, own = pc.precomp_ref(name), pc.own_errors(name)
    edges, sten, ln, wxp = run(name, dev, monkeypatch, literal=False)
    E = len(ref['keep'])
    assert isinstance(sten, FactoredStencil) and sten._dense is None and tuple(sten.shape) == (E, R, F)
    assert np.array_equal(H(edges).astype(np.int64), ref['edges'])
    fac = H(sten.factors)
    assert fac.shape == (E, 8) and not bits(fac[:, 3]).any()
    wrong = np.flatnonzero(bits(fac[:, 0]) != ref['q'])
    assert not len(wrong), 'ring index: (edge, bits of r, device q, restatement q) %s' % [
        (int(e), hex(int(ref['r'][e].astype(np.float32).view(np.int32))), int(bits(fac[:, 0])[e]), int(ref['q'][e])) for e in wrong[:12]]
    c, g = fac[:, 4] + 1j * fac[:, 5], fac[:, 6] + 1j * fac[:, 7]
    assert np.array_equal(bits(fac[:, 4:6]), bits(H(torch.view_as_real(wxp))))
    assert not fac[np.abs(ref['wxp']) == 0][:, 4:6].any()                                 # wxp = 0 in the reference: exactly 0
    got = pc.errors(name, dict(ln=H(ln), wxp=H(wxp), w0=fac[:, 1], w1=fac[:, 2], c=c, g=g))

    # structure: CSR of both sides, slots ordered by (vertex, ring, edge id), the ring-run offsets
    graph = get_graph(edges, sten, N)
    assert graph is sten.graph and graph.factored and (graph.geo_t is not None) == (B >= 1)
    want = pc.graph_ref(ref['edges'], ref['q'], N)
    for key in ('rowptr_t', 'rowptr_s', 'perm_t', 'perm_s', 'nbr_t', 'nbr_s', 'runs_t', 'runs_s'):
        have = H(getattr(graph, key))
        assert have.dtype == want[key].dtype and np.array_equal(have, want[key]), key

    # records: slot order = edge order permuted, bit for bit; word 3 = the other endpoint; padding rows zero
    recf = (4 + 2 * F + 3) // 4 * 4
    rec_t, rec_s = H(graph.rec_t), H(graph.rec_s)
    assert rec_t.shape == rec_s.shape == (E + 1024 // (recf * 4) + 16, recf)
    assert not bits(rec_t[E:]).any() and not bits(rec_s[E:]).any()
    assert np.array_equal(bits(rec_t[:E, 3]), want['nbr_t']) and np.array_equal(bits(rec_s[:E, 3]), want['nbr_s'])
    by_edge = np.empty((E, recf), dtype=np.float32)
    by_edge[want['perm_t']] = rec_t[:E]
    by_edge[:, 3] = 0
    other = rec_s[:E].copy()
    other[:, 3] = 0
    assert np.array_equal(bits(by_edge[want['perm_s']]), bits(other))
    assert np.array_equal(bits(by_edge[:, :3]), bits(fac[:, :3])) and not bits(by_edge[:, 4 + 2 * F:]).any()
    ph = by_edge[:, 4:4 + 2 * F:2] + 1j * by_edge[:, 5:4 + 2 * F:2]
    assert not ph[np.abs(ref['wxp']) == 0].any()
    got['ph'] = pc.errors(name, dict(ph=ph))['ph']
    geo = H(graph.geo_t)
    assert geo.shape == (E + 1024 // 32 + 16, 8) and not bits(geo[E:]).any()
    head = fac[want['perm_t']].copy()
    head[:, 3] = want['nbr_t'].view(np.float32)
    assert np.array_equal(bits(geo[:E]), bits(head))                                   # [q, w0, w1, nbr, c, g] of the same edge

    # the dense rows on demand: from powers of g
    dense = H(sten.materialize())
    check_dense_rows(name, dense, 'sten_exact')
    got['sten_exact'] = pc.errors(name, dict(sten_exact=dense))['sten_exact']
    check('fused %s (E %d of %d, N %d)' % (name, E, pc.case(name)['logMag'].numel(), N), got, own)

    # the literal build of the same inputs: same edges, ln bit-identical
    lit = run(name, dev, monkeypatch, literal=True)
    check_literal(name, lit)
    assert torch.equal(lit[0], edges) and np.array_equal(bits(H(torch.view_as_real(lit[2]))), bits(H(torch.view_as_real(ln))))


@pytest.mark.parametrize('literal', [False, True])
def test_nothing_kept(literal, dev, monkeypatch):
    for form in (torch.int64, torch.int32):
        B, R, eps = pc.CASES['none-kept']
        from fieldconv_amd.transforms import FCPrecomp
        monkeypatch.delenv('FIELDCONV_EAGER_STENCIL', raising=False)
        if literal:
            monkeypatch.setenv('FIELDCONV_EAGER_STENCIL', '1')
        data = pc.support_data('none-kept').to(dev)
        data.supp_edges = data.supp_edges.to(form)
        edges, sten, ln, wxp = FCPrecomp(B, R, eps)(data)
        assert tuple(edges.shape) == (0, 2) and edges.dtype == form
        assert torch.is_tensor(sten) and tuple(sten.shape) == (0, R, 2 * B + 1) and sten.dtype == torch.complex64
        assert tuple(ln.shape) == (0,) and ln.dtype == torch.complex64 and tuple(wxp.shape) == (0,) and wxp.dtype == torch.complex64
        assert all(t.device == data.logMag.device for t in (edges, sten, ln, wxp))


# ---------------------------------------------------------------------------------------------- 2. the literal path
@pytest.mark.parametrize('name', pc.DENSE_CASES)
@pytest.mark.parametrize('literal', [False, True])
def test_literal_path(name, literal, dev, monkeypatch):
    """R * F = 156 fills the LDS of the literal builder; shapes without record-driven kernels return the dense tensor on the default
    path as well"""
    check_literal(name, run(name, dev, monkeypatch, literal))


# ---------------------------------------------------------------------------------------------- 3. fc_graph_build from the dense stencil
def record_errors(rec, sten, perm, q, F):
    """slot-order records against the float64 factorisation of the rows `sten` (E,R,F complex128) with lower ring q: the weights
    (absolute) and the phases (over the row's largest entry), per row"""
    E = len(q)
    rows = np.arange(E)
    s0, s1 = sten[rows, q], sten[rows, q + 1]
    ph = s0 + s1
    den = (np.abs(ph) ** 2).sum(1)
    safe = np.where(den > 0, den, 1.0)
    w0 = np.where(den > 0, (s0 * ph.conj()).sum(1).real / safe, 0.0)
    w1 = np.where(den > 0, (s1 * ph.conj()).sum(1).real / safe, 0.0)
    r = rec[:E].astype(np.float64)
    got_ph = r[:, 4:4 + 2 * F:2] + 1j * r[:, 5:4 + 2 * F:2]
    scale = np.abs(sten).reshape(E, -1).max(axis=1)[perm]
    one = np.ones(E)
    return dict(w0=pc.per_edge_err(r[:, 1], w0[perm], one), w1=pc.per_edge_err(r[:, 2], w1[perm], one),
                ph=pc.per_edge_err(got_ph, ph[perm], scale))


def geo_errors(geo, sten, perm, q, F):
    E, B = len(q), (F - 1) // 2
    ph = sten[np.arange(E), q] + sten[np.arange(E), q + 1]
    live = np.abs(ph[:, B]) > 0
    g = np.where(live, ph[:, min(B + 1, F - 1)] / np.where(live, ph[:, B], 1.0), 1.0)
    r = geo[:E].astype(np.float64)
    scale = np.abs(sten).reshape(E, -1).max(axis=1)[perm]
    return dict(c=pc.per_edge_err(r[:, 4] + 1j * r[:, 5], ph[perm, B], scale), g=pc.per_edge_err(r[:, 6] + 1j * r[:, 7], g[perm], np.ones(E)))


def both_builds(edges, sten, N):
    from fieldconv_amd.graph import SupportGraph
    return SupportGraph(edges, sten, N, native=True), SupportGraph(edges, sten, N, native=False)


def assert_same_structure(a, b, E):
    for key in ('rowptr_t', 'rowptr_s', 'perm_t', 'perm_s', 'nbr_t', 'nbr_s'):
        x, y = getattr(a, key), getattr(b, key)
        assert x.dtype == y.dtype and torch.equal(x, y), key
    assert a.factored == b.factored and (a.geo_t is None) == (b.geo_t is None)
    if a.factored:
        assert torch.equal(a.runs_t, b.runs_t) and torch.equal(a.runs_s, b.runs_s)
        for key in ('rec_t', 'rec_s') + (('geo_t',) if a.geo_t is not None else ()):
            x, y = H(getattr(a, key)), H(getattr(b, key))
            assert x.shape == y.shape and np.array_equal(bits(x[:, 0]), bits(y[:, 0])) and np.array_equal(bits(x[:, 3]), bits(y[:, 3])), key
            assert not bits(x[E:]).any()


@pytest.mark.parametrize('name', pc.GRAPH_CASES + ('B0-R6',))
def test_graph_build_from_dense_stencil(name, dev):
    """fc_graph_build against the torch build of graph.py on the CPU oracle's stencil: knot-exact rows (one non-zero ring), all-zero
    rows (areas), runs of 31 / 32 / 33 / 64 edges, more long runs than the long-run kernel has workgroups; `B0-R6`: F = 1, 8-float
    records, no geometric form.  Records per row against the float64 factorisation of the same rows; gate = 4 x the torch build's
    own error, floor 1e-6.
    The ring index handed to graph_ref is the restatement's only where the stencil shows it (`seen`: the edge has weight, its lower
    ring is non-zero, its radius is not a planted one).  A dense row on a knot, without weight or next to a knot does not tell its
    lower ring; there q is read from the native records, and the torch build, bit for bit, is the only witness."""
    from fieldconv_amd.graph import _native_build, factor_stencil
    B, R, eps = pc.CASES[name]
    F, N = 2 * B + 1, pc.case(name)['N']
    ref, f32 = pc.precomp_ref(name), pc.precomp_f32(name)
    E = len(ref['keep'])
    edges, sten = torch.from_numpy(ref['edges']).to(dev), torch.from_numpy(f32['sten']).to(dev)
    sten64 = f32['sten'].astype(np.complex128)
    if B == 0:          # no convolution kernels for this shape: the build itself, with records
        nat = _native_build(edges, sten, N, R, F, True, False)
        assert nat['flags'] == 0
        rec = factor_stencil(sten)
        q = H(rec[:, 0].view(torch.int32)).astype(np.int64)
        want = pc.graph_ref(ref['edges'], q, N)
        for key in ('rowptr_t', 'rowptr_s', 'perm_t', 'perm_s', 'nbr_t', 'nbr_s', 'runs_t', 'runs_s'):
            assert np.array_equal(H(nat[key]), want[key]), key
        for side in 'ts':
            perm, r = want['perm_' + side], H(nat['rec_' + side])
            assert r.shape[1] == 8 and np.array_equal(bits(r[:E, 0]), q[perm].astype(np.int32)) and np.array_equal(bits(r[:E, 3]), want['nbr_' + side])
            own = record_errors(H(rec)[perm], sten64, perm, q, F)
            check('graph build %s rec_%s' % (name, side), record_errors(r, sten64, perm, q, F), own)
        return
    nat, tor = both_builds(edges, sten, N)
    assert nat.factored and tor.factored and nat.geo_t is not None
    assert_same_structure(nat, tor, E)
    q = np.empty(E, dtype=np.int64)
    q[H(nat.perm_t)] = bits(H(nat.rec_t)[:E, 0])
    seen = (np.abs(ref['wxp']) > 0) & (ref['w0'] > 0) & ~pc.knot_neighbour(name)          # the stencil shows the lower ring
    assert np.array_equal(q[seen], ref['q'][seen])
    want = pc.graph_ref(ref['edges'], q, N)
    for key in ('rowptr_t', 'rowptr_s', 'perm_t', 'perm_s', 'nbr_t', 'nbr_s', 'runs_t', 'runs_s'):
        assert np.array_equal(H(getattr(nat, key)), want[key]), key
    for side in 'ts':
        perm = want['perm_' + side]
        assert np.array_equal(bits(H(getattr(nat, 'rec_' + side))[:E, 3]), want['nbr_' + side])
        own = record_errors(H(getattr(tor, 'rec_' + side)), sten64, perm, q, F)
        check('graph build %s rec_%s' % (name, side), record_errors(H(getattr(nat, 'rec_' + side)), sten64, perm, q, F), own)
    check('graph build %s geo_t' % name, geo_errors(H(nat.geo_t), sten64, want['perm_t'], q, F),
          geo_errors(H(tor.geo_t), sten64, want['perm_t'], q, F))


# ---------------------------------------------------------------------------------------------- 4. row scaling of a valid stencil
def rebuilt_rows(graph, E, R, F):
    """(E,R,F) complex128 in edge order from the factored records of the graph: w_q ph in ring q, w_{q+1} ph in ring q + 1"""
    rec, perm = H(graph.rec_t)[:E].astype(np.float64), H(graph.perm_t)
    q = bits(H(graph.rec_t)[:E, 0]).astype(np.int64)
    ph = rec[:, 4:4 + 2 * F:2] + 1j * rec[:, 5:4 + 2 * F:2]
    rows = np.zeros((E, R, F), dtype=np.complex128)
    rows[np.arange(E), q] = rec[:, 1:2] * ph
    rows[np.arange(E), q + 1] += rec[:, 2:3] * ph
    out = np.empty_like(rows)
    out[perm] = rows
    return out


def test_row_scaling_of_a_valid_stencil(dev):
    """The `areas` stencil with every row times 2^s, s in -70 .. 20: still rank-1, two-ring, geometric, rows between 2^-110 and 2^20.
    Either a build factors it and its records give the rows back per row, or it reports a dense stencil and carries the rows; both
    builds reach the same verdict, and the convolution over the native graph matches the oracle on the scaled stencil row by row.
    (A build that squares the entries before it compares them takes rows below 2^-63 for empty.)"""
    from fieldconv_amd.functional import field_conv
    name = 'areas'
    B, R, eps = pc.CASES[name]
    F, N = 2 * B + 1, pc.case(name)['N']
    ref, f32 = pc.precomp_ref(name), pc.precomp_f32(name)
    E = len(ref['keep'])
    factor = np.ldexp(1.0, pc.row_exponents(name)).astype(np.float32)
    scaled = f32['sten'] * factor[:, None, None]
    assert scaled.dtype == np.complex64
    exact = f32['sten'].astype(np.complex128) * factor.astype(np.float64)[:, None, None]
    assert np.abs(scaled - exact).max() <= 2.0 ** -149                      # powers of two: exact, bar the float32 denormals
    row_scale = np.abs(exact).reshape(E, -1).max(axis=1)
    assert row_scale[row_scale > 0].min() < 2.0 ** -90 and row_scale.max() > 2.0 ** 10
    edges, sten = torch.from_numpy(ref['edges']).to(dev), torch.from_numpy(scaled).to(dev)
    nat, tor = both_builds(edges, sten, N)
    gate = pc.gate_of(pc.own_errors(name)['sten'])
    for label, g in (('native', nat), ('torch', tor)):
        if g.factored:
            err = pc.per_edge_err(rebuilt_rows(g, E, R, F), exact, row_scale)
            print('\nrow scaling, %s build: factored, rows from the records %.2e (gate %.2e)' % (label, err, gate))
            assert err <= gate, (label, err)
        else:
            print('\nrow scaling, %s build: dense' % label)
            assert g.sten_t is not None and torch.equal(torch.view_as_real(g.sten_t), torch.view_as_real(sten[g.perm_t]))
    assert nat.factored == tor.factored and (nat.geo_t is None) == (tor.geo_t is None)
    if nat.factored:                    # (dense: any order inside a vertex serves)
        assert_same_structure(nat, tor, E)

    I = O = 4
    gen = torch.Generator().manual_seed(5)
    x = torch.complex(torch.randn(N, I, generator=gen), torch.randn(N, I, generator=gen))
    W = torch.complex(torch.randn(O, I, R, F, generator=gen), torch.randn(O, I, R, F, generator=gen)) / (I * R) ** 0.5
    y = field_conv(x.to(dev), W.to(dev), nat)
    y_ref = orc.fieldconv_forward(x.numpy().astype(np.complex128), ref['edges'], exact, W.numpy().astype(np.complex128))
    err = measured_err(H(y), y_ref)
    print('row scaling: convolution over the native graph, row-wise %.2e (gate %.2e)' % (err, CONV_TOL))
    assert np.isfinite(H(torch.view_as_real(y))).all() and err < CONV_TOL


@pytest.mark.parametrize('value', [float('inf'), float('nan')])
def test_row_with_a_non_finite_entry_does_not_factor(value, dev):
    """one infinite or NaN entry in an otherwise valid stencil: neither build factors it (values, not faults)"""
    name = 'areas'
    N = pc.case(name)['N']
    ref, f32 = pc.precomp_ref(name), pc.precomp_f32(name)
    sten = torch.from_numpy(f32['sten'].copy())
    e = int(np.flatnonzero(np.abs(ref['wxp']) > 0)[3])
    sten[e, int(ref['q'][e]), 1] = complex(value, 0.0)
    nat, tor = both_builds(torch.from_numpy(ref['edges']).to(dev), sten.to(dev), N)
    assert not nat.factored and not tor.factored and nat.rec_t is None and nat.sten_t is not None
    assert torch.equal(nat.rowptr_t, tor.rowptr_t) and torch.equal(nat.rowptr_s, tor.rowptr_s)          # (dense: any order inside a vertex)


# ---------------------------------------------------------------------------------------------- 5. errors
@pytest.mark.parametrize('literal', [False, True])
def test_vertex_id_out_of_range(literal, dev, monkeypatch):
    """a kept edge that refers to a vertex >= N raises IndexError on both paths; the same id on a dropped edge (beyond epsilon, or NaN)
    does not: dropped edges are never looked at"""
    from fieldconv_amd.transforms import FCPrecomp
    name = 'gap'
    B, R, eps = pc.CASES[name]
    c, ref = pc.case(name), pc.precomp_ref(name)
    monkeypatch.delenv('FIELDCONV_EAGER_STENCIL', raising=False)
    if literal:
        monkeypatch.setenv('FIELDCONV_EAGER_STENCIL', '1')
    mag = c['logMag'].numpy()
    beyond = int(np.flatnonzero(np.isfinite(mag) & (mag > eps))[0])
    nan = int(np.flatnonzero(np.isnan(mag))[0])
    for e, col, raises in ((beyond, 0, False), (nan, 1, False), (int(ref['keep'][0]), 1, True), (int(ref['keep'][-1]), 0, True)):
        data = pc.support_data(name).to(dev)
        bad = data.supp_edges.clone()
        bad[e, col] = c['N'] + 3
        data.supp_edges = bad
        if raises:
            with pytest.raises(IndexError):
                FCPrecomp(B, R, eps)(data)
        else:
            out = FCPrecomp(B, R, eps)(data)
            assert np.array_equal(H(out[0]), ref['edges'])
