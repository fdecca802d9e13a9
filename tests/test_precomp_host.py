"""_precomp_cases.py on the CPU: the float64 restatement of FCPrecomp (precomp_ref) against the oracle's float32 restatement on every
planted case -- identical kept edges, the same two rings, values within float32 rounding, every edge compared -- the structural
restatement (graph_ref) against the torch build of fieldconv_amd.graph, and the planted properties themselves: radii on the knots and
one ulp to either side, run lengths around kShortRun, more long runs than graph_order_long_kernel has workgroups, workgroups that keep
nothing, the vertex whose area sum is zero.

The float32 restatement's own per-edge errors, printed here, are what test_gpu_precomp.py derives its gates from (4 x, floor 1e-6)."""
import numpy as np
import pytest
import torch

import _precomp_cases as pc

def f32_rounding(R):
    """What the float32 restatement may differ by, per edge: 8 roundings of 2^-24 in the products, and in the interpolation weight
    (r - k_lo) / (k_hi - k_lo) the roundings of r, of the difference and of the two knots (torch.sqrt: up to one ulp each), 4 ulps of
    2^-24 in all over the narrowest ring, 1 - sqrt(1 - 1 / (R-1))."""
    return 2.0 ** -24 * (8 + 4 / (1 - np.sqrt(1 - 1 / (R - 1))))


@pytest.mark.parametrize('name', list(pc.CASES))
def test_restatement_agrees_with_float32_oracle(name):
    c, ref, f32 = pc.case(name), pc.precomp_ref(name), pc.precomp_f32(name)
    B, R, eps = pc.CASES[name]
    assert c['N'] <= 700 and c['logMag'].numel() <= 25000
    # the division that decides the kept edges and the rings is the same IEEE float32 division everywhere
    r_np = c['logMag'].numpy() / np.float32(eps)
    assert np.array_equal((c['logMag'] / eps).numpy().view(np.int32), r_np.view(np.int32))
    assert np.array_equal(np.flatnonzero(r_np <= 1), ref['keep'])
    assert np.array_equal(ref['edges'], f32['edges']) and f32['edges'].dtype == np.int64
    assert not np.isin(np.flatnonzero(~np.isfinite(c['logMag'].numpy())), ref['keep']).any()          # inf and NaN are dropped
    E = len(ref['keep'])
    assert f32['sten'].shape == (E, R, 2 * B + 1) and ref['sten'].shape == (E, R, 2 * B + 1)
    if name == 'none-kept':
        assert E == 0
        return
    assert E > 0
    # the same upper knot: the oracle's weights sit in columns q, q + 1 and nowhere else, for every edge that is not planted on a knot
    # or next to one (there the oracle's ring follows the CPU's square root, see _precomp_cases.knots32; the VALUES below are compared
    # for every edge all the same: the interpolation is continuous across a knot)
    ring = f32['ring']
    inside = np.zeros_like(ring, dtype=bool)
    inside[np.arange(E), ref['q']] = inside[np.arange(E), ref['q'] + 1] = True
    knot_neighbour = pc.knot_neighbour(name)
    assert not ring[~knot_neighbour][~inside[~knot_neighbour]].any()
    assert np.abs(pc.knots32(R).numpy().view(np.int32) - torch.sqrt(torch.arange(R) / (R - 1)).numpy().view(np.int32)).max() <= 1
    both = (ring[np.arange(E), ref['q']] != 0) & (ring[np.arange(E), ref['q'] + 1] != 0)
    assert both[~knot_neighbour].all()
    live = np.abs(ref['wxp']) > 0
    assert np.array_equal((np.abs(f32['sten']).max(axis=2) > 0)[live & ~knot_neighbour], (ring != 0)[live & ~knot_neighbour])
    assert not (np.abs(f32['sten']).max(axis=2) > 0)[~knot_neighbour][~inside[~knot_neighbour]].any()
    assert not f32['sten'][~live].any() and not ref['sten'][~live].any()
    assert np.allclose(ref['w0'] + ref['w1'], 1.0, atol=1e-15)
    own = pc.own_errors(name)
    print('\n%s: E %d kept %d; float32 restatement per edge: %s' % (name, c['logMag'].numel(), E, '  '.join('%s %.2e' % kv for kv in sorted(own.items()))))
    assert all(e <= f32_rounding(R) for e in own.values()), own
    # the rows with m * theta in float64 differ from the reference's by the rounding of that product alone
    m = np.arange(-B, B + 1)
    theta = c['logAng'].numpy()[ref['keep']]
    prod32 = m[None, :].astype(np.float32) * theta[:, None]
    assert prod32.dtype == np.float32
    slack = np.abs(prod32.astype(np.float64) - m[None, :].astype(np.float64) * theta[:, None].astype(np.float64)).max(axis=1)
    diff = np.abs(ref['sten_exact'] - ref['sten']).reshape(E, -1).max(axis=1)
    assert np.all(diff <= (slack * 1.0000001 + 1e-15) * np.abs(ref['wxp']))
    if B <= 2:
        assert slack.max() == 0                 # products with 0, +-1, +-2 are exact


@pytest.mark.parametrize('name', ['knots-R2-e1', 'knots-R3-e03', 'knots-R6-e1', 'knots-R6-e03', 'knots-R8-e03', 'literal-R12-B6'])
def test_planted_radii_reach_the_knots(name):
    """Every knot is hit exactly, and from both sides, in r = logMag / eps as the builders compute it; so are 0, eps and the support's
    boundary (kept at r = 1, dropped one ulp above), and the planted angles are there."""
    c, ref = pc.case(name), pc.precomp_ref(name)
    B, R, eps = pc.CASES[name]
    r = (c['logMag'] / torch.tensor(eps, dtype=torch.float32)).numpy()
    k = pc.knots32(R).numpy()
    for q in range(R):
        near = r[np.abs(r - k[q]) <= 4 * np.spacing(k[q])] if q else r[np.abs(r) <= 1e-44]
        assert len(near) >= 6 and len(set(near)) >= 2, (q, near)
        if eps == 1.0 or q == 0:            # (a power of two: r IS logMag; otherwise the quotient lands where the division puts it)
            assert (near == k[q]).any() and (near < k[q]).any() and (near > k[q]).any(), (q, near)
    kept = np.zeros(len(r), dtype=bool)
    kept[ref['keep']] = True
    assert kept[r == 1].all() and (r == 1).any() and not kept[r > 1].any() and (r == np.nextafter(np.float32(1), np.float32(2))).any()
    on_knot = np.isin(ref['r'].astype(np.float32), k[1:])
    assert on_knot.sum() >= R - 1
    assert np.all(ref['w1'][on_knot] == 1.0) and np.all(ref['w0'][on_knot] == 0.0)         # on a knot: the upper ring alone
    assert np.all(ref['q'][ref['r'] <= 0] == 0) and (ref['r'] < 0).any()
    assert np.isin(pc.planted_angles(), c['logAng'].numpy()).all()


def test_planted_structure():
    W = pc.WORKGROUP
    for name in [n for n in pc.CASES if n.startswith('sizes')]:
        assert pc.case(name)['logMag'].numel() == int(name[len('sizes-E'):]) and len(pc.precomp_ref(name)['keep']) >= 1
    keep = pc.precomp_ref('gap')['keep']
    assert not ((keep >= W) & (keep < 3 * W)).any() and (keep == W - 1).any() and (keep == 3 * W).any() and (keep > 3 * W).any()
    assert pc.case('gap')['logMag'].numel() > 4 * W and pc.case('gap')['logMag'].numel() % W
    assert len(pc.precomp_ref('none-kept')['keep']) == 0

    c, ref = pc.case('areas'), pc.precomp_ref('areas')
    w = c['w'].numpy()[:, 0]
    assert w.max() == 1.0 and w[w > 0].min() == 2.0 ** -40 and not w[list(pc.AREAS_ZERO_SOURCES)].any()
    src, dst = ref['edges'][:, 0], ref['edges'][:, 1]
    into = dst == pc.AREAS_ZERO_TOTAL
    assert into.sum() >= 3 and np.isin(src[into], pc.AREAS_ZERO_SOURCES).all()
    assert ref['total'][pc.AREAS_ZERO_TOTAL] == 0 and not ref['wxp'][into].any() and not ref['sten'][into].any()
    assert np.isin(src, pc.AREAS_ZERO_SOURCES).sum() > into.sum()                # zero-area sources also feed targets with area
    all_src, all_dst = c['supp_edges'][:, 0].numpy(), c['supp_edges'][:, 1].numpy()
    assert (all_dst == pc.AREAS_NO_IN).any() and not (dst == pc.AREAS_NO_IN).any()
    assert (all_src == pc.AREAS_NO_OUT).any() and not (src == pc.AREAS_NO_OUT).any()
    assert np.abs(ref['wxp'])[np.abs(ref['wxp']) > 0].min() < 2.0 ** -30

    for name in ('dups-i32', 'dups-T'):
        ref = pc.precomp_ref(name)
        pairs, counts = np.unique(ref['edges'], axis=0, return_counts=True)
        assert (counts >= 3).sum() >= 3
        for s, d in ((3, 7), (7, 3), (9, 9)):
            same = (ref['edges'][:, 0] == s) & (ref['edges'][:, 1] == d)
            assert same.sum() >= 3 and len(set(ref['q'][same])) >= 2

    ref = pc.precomp_ref('runs-32-33')
    g = pc.graph_ref(ref['edges'], ref['q'], pc.case('runs-32-33')['N'])
    for t, length in enumerate(pc.RUN_LENGTHS):
        assert g['hist_t'][t, t % 5] == length and g['hist_t'][t, (t + 2) % 5] == 3
        assert g['hist_s'][4 + t, t % 5] == length and g['hist_s'][4 + t, (t + 2) % 5] == 3
    assert pc.SHORT_RUN in pc.RUN_LENGTHS and pc.SHORT_RUN + 1 in pc.RUN_LENGTHS and pc.SHORT_RUN - 1 in pc.RUN_LENGTHS

    c, ref = pc.case('many-long-runs'), pc.precomp_ref('many-long-runs')
    assert len(ref['keep']) == c['logMag'].numel() <= 25000
    g = pc.graph_ref(ref['edges'], ref['q'], c['N'])
    for side in 'ts':
        long_runs = g['hist_' + side][g['hist_' + side] > pc.SHORT_RUN]
        assert len(long_runs) >= 300 > pc.LONG_WORKGROUPS and long_runs.min() >= 33 and long_runs.max() <= 40
        assert set(long_runs) == set(pc.LONG_RUN_LENGTHS)
    assert not np.array_equal(np.sort(ref['edges'][:, 1], kind='stable'), ref['edges'][:, 1])       # the edge order is a permutation


@pytest.mark.parametrize('name', pc.GRAPH_CASES + ('dups-T', 'gap'))
def test_graph_ref_agrees_with_torch_build(name):
    """graph_ref against the torch build (fieldconv_amd.graph: stable sorts, bincount, cumsum) on the float32 oracle's stencil, with
    the ring index of the restatement wherever the stencil shows it (an edge on a knot has one non-zero ring, an edge without weight
    none: the dense build cannot know their lower ring; see GRAPH cases of test_gpu_precomp.py)."""
    from fieldconv_amd.graph import factor_stencil
    c, ref, f32 = pc.case(name), pc.precomp_ref(name), pc.precomp_f32(name)
    sten = torch.from_numpy(f32['sten'])
    rec = factor_stencil(sten)
    assert rec is not None
    q = rec[:, 0].view(torch.int32).numpy()
    seen = (np.abs(ref['wxp']) > 0) & (ref['w0'] > 0) & ~pc.knot_neighbour(name)
    assert np.array_equal(q[seen], ref['q'][seen])
    g = pc.graph_ref(ref['edges'], q, c['N'])
    edges = torch.from_numpy(ref['edges'])
    for side, key, other in (('t', edges[:, 1], edges[:, 0]), ('s', edges[:, 0], edges[:, 1])):
        _, perm = torch.sort(key * c['R'] + torch.from_numpy(q).long(), stable=True)
        assert np.array_equal(perm.numpy(), g['perm_' + side]) and np.array_equal(other[perm].numpy(), g['nbr_' + side])
        assert g['rowptr_' + side][-1] == len(q) and np.array_equal(np.diff(g['rowptr_' + side]), np.bincount(key.numpy(), minlength=c['N']))
        assert np.array_equal(g['runs_' + side][:, 1:], np.cumsum(g['hist_' + side], 1)[:, :-1])
    # the records the restatement predicts, against factor_stencil's (float32): weights and phases per edge
    want = pc.record_ref(name)
    F = 2 * c['B'] + 1
    mag = np.abs(ref['wxp'])
    got = rec.numpy().astype(np.float64)
    assert pc.per_edge_err(got[seen][:, 4:4 + 2 * F], want[seen][:, 4:], mag[seen]) <= f32_rounding(c['R'])
    assert pc.per_edge_err(got[seen][:, 1:3], want[seen][:, 1:3], np.ones(int(seen.sum()))) <= f32_rounding(c['R'])
