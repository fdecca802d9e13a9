"""Pins the inputs of the TransField / ECHO row-wise tests (_lift_echo_cases.py) on the CPU, so that test_gpu_lift_echo.py cannot hide
a failure behind its own inputs, masks or gates:

  * the planted meshes carry the row lengths, wavefront counts and partly filled workgroups they are named for;
  * every scaled input is exact in fp32, and the directly evaluated float64 reference equals the unscaled one times 2^a_n;
  * the float32 restatement stays below 1e-4 row-wise on y and desc (and, with the seeds chosen, on every gradient), so that
    the gate -- 4 x that error, floor 1e-6 -- cannot become vacuous;
  * no row is unmeasurably small, no A sits next to the origin box, and the fragile votes and near-box histogram entries that
    are left out stay under their cap;
  * the rows that containment compares are at least half of all rows."""
import numpy as np
import pytest

import _lift_echo_cases as lc

OWN_MAX = 1e-4
TF_ALL = list(lc.TF_CASES) + list(lc.TF_CONTAINMENT)
ECHO_ALL = list(lc.ECHO_CASES) + list(lc.ECHO_CONTAINMENT)


def test_waves_per_vertex_restates_both_launchers():
    import os
    import re
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'fieldconv_amd', 'csrc')
    for fname, fn in (('fc_trans_field.hip', 'tf_waves_per_vertex'), ('fc_echo.hip', 'echo_waves_per_vertex')):
        body = re.search(r'static int %s\(int N, int E\) \{(.*?)\n\}' % fn, open(os.path.join(root, fname)).read(), re.S).group(1)
        assert 'deg >= 64 && N < 65536) return 4' in body and 'deg >= 32 && N < 131072) return 2' in body and '(long)E / N' in body, fname
    assert [lc.waves_per_vertex(10, e) for e in (319, 320, 639, 640)] == [1, 2, 2, 4]


@pytest.mark.parametrize('ahead', [lc.TF_AHEAD, lc.ECHO_AHEAD])
def test_planted_meshes(ahead):
    for name, (N, D, planted, quiet) in lc.MESHES.items():
        edges, no_out = lc.mesh(name, ahead)
        E = edges.shape[0]
        assert E // N == D and edges.min() >= 0 and edges.max() < N
        wpv = lc.waves_per_vertex(N, E)
        deg = lc.in_degrees(name, ahead)
        if no_out is not None:
            assert not (edges[:, 0] == no_out).any()
        if planted:
            assert set(lc.planted_degrees(wpv, ahead)) <= set(deg.tolist()), name
        if quiet:
            P = lc.perturbed_set(N)
            assert P.size >= 2 and np.all(P % lc.WPG == lc.WPG - 1) and np.all(deg[P] == 3)
            assert np.all(np.bincount(edges[:, 0], minlength=N)[P] == 2)
            fwd, bwd = lc.affected_rows(edges, N, P)
            assert (~fwd).mean() >= 0.5 and (~bwd).mean() >= 0.5, name          # containment compares at least half of the rows
    wpv = {name: lc.waves_per_vertex(lc.MESHES[name][0], lc.mesh(name, ahead)[0].shape[0]) for name in lc.MESHES}
    assert (wpv['w1-31'], wpv['w2-32'], wpv['w2-63'], wpv['w4-64'], wpv['quiet1'], wpv['quiet2']) == (1, 2, 2, 4, 1, 2)
    assert [lc.MESHES[m][1] for m in ('w1-31', 'w2-32', 'w2-63', 'w4-64')] == [31, 32, 63, 64]          # either side of both thresholds
    assert sorted(lc.MESHES[m][0] % 4 for m in ('w1-31', 'n42', 'n43')) == [1, 2, 3] and lc.MESHES['w2-32'][0] % 2 == lc.MESHES['w2-63'][0] % 2 == 1
    # the TransField backward plan: persistent wavefronts = a quarter of the vertices in whole workgroups below N = 4096, 1024 from there
    waves = lambda N: ((N + 3) // 4 + 3) // 4 * 4 if N < 4096 else 1024
    assert (waves(37) % 16, waves(4095), waves(4099)) == (12, 1024, 1024)


@pytest.mark.parametrize('layout', lc.LAYOUTS)
def test_exponent_layouts(layout):
    for N in sorted({m[0] for m in lc.MESHES.values()}):
        a = lc.exponents(N, layout, -8, 8)
        assert a.min() >= -8 and a.max() <= 8 and a.shape == (N,)
        groups = [a[b:b + lc.WPG] for b in range(0, N, lc.WPG)]
        if layout == 'random':
            assert a[N - 1] == -8
            assert all(g.max() == 8 and g.min() == -8 for g in groups if g.size == lc.WPG)
        else:
            assert all(np.all(g == (8 if k % 2 == 0 else -8)) for k, g in enumerate(groups))


def test_case_tables_are_what_the_issue_lists():
    zm = [lc.tf_case(n) for n in lc.ZERO_MAGNITUDE_CASES]          # lane-mapped float32, run-time float32, run-time float64
    assert [lc.tf_specialised(*c[1:4], c[6]) for c in zm] == [True, False, False] and [c[6] for c in zm] == [False, False, True]
    sizes = {lc.tf_case(n)[1:4] for n in lc.TF_CASES if n.startswith('size-')}
    assert sizes == {(4, 8, 64), (1, 1, 1), (3, 6, 48), (5, 6, 16), (3, 9, 16), (3, 6, 65)}
    assert all(lc.tf_specialised(*s, False) for s in lc.TF_SPECIALISED_SIZES) and not any(lc.tf_specialised(*s, False) for s in lc.TF_GENERIC_SIZES)
    assert {lc.tf_case(n)[4] for n in lc.TF_CASES if n.startswith('size-')} == {0, 1} and lc.TF_CASES['f64'][6]
    assert [lc.TF_CASES[n][1:4] for n in ('plan37', 'plan4095', 'plan4099')] == [(3, 6, 16)] * 3
    assert [lc.channel_block(b) for b in range(1, 9)] == [64, 64, 64, 64, 57, 42, 30, 23]          # include/fieldconv_hip.h
    for nb in (1, 3, 5, 8):
        want = {lc.channel_block(nb), lc.channel_block(nb) + 1, 64, 65}
        assert {lc.ECHO_CASES[n][1] for n in lc.ECHO_CASES if n.startswith('blocks-b%d-' % nb)} == want
    assert lc.ECHO_CASES['bins9'][2] == 9 and lc.ECHO_CASES['c128'][4]


def test_channel_block_matches_the_library():
    from fieldconv_amd import _lib
    lib = _lib.load()
    for nb in range(1, 9):
        assert lib.fc_echo_channel_block(nb) == lc.channel_block(nb) and lib.fc_echo_hist_dim(nb) == lc.hist_dim(nb)


def fp32_exact(t, t0, f):
    """t (complex64 / float32) equals t0 times the powers of two f, formed in double precision"""
    wide = np.complex128 if np.iscomplexobj(t) else np.float64
    real = t.view(np.float32) if np.iscomplexobj(t) else t
    return np.isfinite(real).all() and np.array_equal(t.astype(wide), t0.astype(wide) * f)


@pytest.mark.parametrize('name', TF_ALL)
def test_trans_field_inputs_and_reference(name):
    m, Cin, R, O, ftype, layout, f64 = lc.tf_case(name)
    p, p0 = lc.tf_problem(name), lc.tf_problem(name, scaled=False)
    N = lc.MESHES[m][0]
    a = lc.tf_exponents(name)
    f = np.ldexp(1.0, a)[p['edges'][:, 1]]
    # -- exact scaling; the factor table stands for the same two columns
    assert p['s01'].dtype == np.complex64 and fp32_exact(p['s01'], p0['s01'], f[:, None, None])
    if p['factors'] is not None:
        fac = p['factors'].astype(np.float64)
        q = p['factors'][:, 0].view(np.int32)
        ring = np.zeros((f.size, R))
        ring[np.arange(f.size), q], ring[np.arange(f.size), q + 1] = fac[:, 1], fac[:, 2]
        c, g = fac[:, 4] + 1j * fac[:, 5], fac[:, 6] + 1j * fac[:, 7]
        s0 = ring * c[:, None]
        assert np.array_equal(np.stack((s0, s0 * g[:, None]), 2).astype(np.complex64), p['s01'])
    else:
        assert R == 1
    # -- stencil entries: exact zeros, or outside the origin box by a factor of 10 at every exponent
    big = np.maximum(np.abs(p['s01'].real), np.abs(p['s01'].imag))
    assert (big == 0).any() or R == 1
    assert big[big > 0].min() > lc.BOX_HI
    # -- the planted exactly-zero magnitude: in-edges, zero sources in that channel, a live angular part
    zm = lc.zero_magnitude_entry(name)
    assert (zm is not None) == (name in lc.ZERO_MAGNITUDE_CASES)
    if zm is not None:
        n, i = zm
        srcs = p['edges'][p['edges'][:, 1] == n, 0]
        assert srcs.size > 0 and np.all(p['x'][srcs, i] == 0) and p['x'][n, i] != 0
        assert np.abs(lc.tf_A(name)[n, :, i]).min() > 0
    # -- condition 3: no A next to the box
    assert not lc.near_box(lc.tf_A(name)).any()
    # -- the reference scales exactly
    r64, r0 = lc.tf_reference(name), lc.tf_reference(name, 'f64', scaled=False)
    assert np.array_equal(r64['y'], r0['y'] * np.ldexp(1.0, a)[:, None])
    deg = lc.in_degrees(m, lc.TF_AHEAD)
    if lc.MESHES[m][2]:
        assert (deg == 0).any() and np.all(r64['y'][deg == 0] == 0)          # zero rows stay in, and must come out as zeros
    # -- conditions 1 and 2
    own = lc.tf_errors(lc.tf_reference(name, 'f32'), r64)
    assert set(own) == set(r64) - ({'g_zonalAng'} if R == 1 else set())
    assert all(e <= OWN_MAX for e in own.values()), own
    for k, t in r64.items():
        assert np.isfinite(t.astype(np.complex64 if np.iscomplexobj(t) else np.float32).view(np.float32)).all()
        assert lc.excluded_rows(t).mean() <= lc.MAX_EXCLUDED, k


@pytest.mark.parametrize('name', ECHO_ALL)
def test_echo_inputs_and_reference(name):
    m, C, n_bins, layout, c128 = lc.echo_case(name)
    p, p0 = lc.echo_problem(name), lc.echo_problem(name, scaled=False)
    N = lc.MESHES[m][0]
    a = lc.echo_exponents(name)
    assert p['wxp'].dtype == np.complex64 and fp32_exact(p['wxp'], p0['wxp'], np.ldexp(1.0, a)[p['edges'][:, 1]])
    assert all(np.array_equal(p[k], p0[k]) for k in ('edges', 'ln', 'x', 'gd'))
    assert np.abs(p['ln']).max() < 0.99 and (p['ln'] == 0).any()
    zero = p['x'] == 0
    assert N == 1 or (0.02 < zero.mean() < 0.12 and zero[lc.ZERO_X_ROW].all())
    # features are exact zeros or far outside the origin box
    big = np.maximum(np.abs(p['x'].real), np.abs(p['x'].imag))
    assert big[~zero].min() > lc.BOX_HI
    # -- the reference scales exactly wherever neither side is inside the origin box; an entry that crosses the box is tiny
    r64, r0 = lc.echo_reference(name), lc.echo_reference(name, 'f64', scaled=False)
    resc = r0['desc'] * np.ldexp(1.0, a)[:, None, None]
    both = (resc > 0) & (r64['desc'] > 0)
    assert np.array_equal(r64['desc'][both], resc[both])
    assert np.maximum(resc, r64['desc'])[~both].max(initial=0.0) < np.sqrt(2.0) * 1e-7 * 2.0 ** lc.ECHO_RANGE[1]
    deg = lc.in_degrees(m, lc.ECHO_AHEAD)
    if lc.MESHES[m][2]:
        assert (deg == 0).any() and np.all(r64['desc'][deg == 0] == 0)
    # -- conditions 3 and 4: what is left out, under the cap
    ok, okg, share = lc.echo_masks(name)
    # The cap of the issue holds for the descriptor entries.  A gradient entry gx[j,c] is left out when ANY out-edge of j votes into a
    # left-out entry of channel c: with k out-edges and four bins per vote that is about 4 k times the descriptor share -- 0.0027 * 4 * 63
    # would be 0.7 if every vote hit another bin; measured at most 0.14 (rows-w2-63), a few per cent at k = 6.  Cap: 0.15.
    assert share < lc.MAX_FRAGILE and okg.mean() > 0.85, (share, okg.mean())
    # -- conditions 1 and 2
    own = lc.echo_errors(name, lc.echo_reference(name, 'f32'), r64)
    assert max(own) <= OWN_MAX, own
    assert lc.excluded_rows(r64['desc'] * ok).mean() <= lc.MAX_EXCLUDED and lc.excluded_rows(r64['gx'] * okg).mean() <= lc.MAX_EXCLUDED


def test_gate_has_a_floor_and_follows_the_restatement():
    assert lc.gate_of(0.0) == 1e-6 and lc.gate_of(1e-5) == 4e-5 and lc.gate_of(1e-5, f64=True) == 1e-12
