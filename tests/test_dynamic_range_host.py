"""Pins the generator of the row-by-row dynamic-range tests (_dynamic_range_cases.py) on the CPU, so that a GPU test
built on it cannot hide a failure behind its own inputs: the scaled inputs are exact, the rescaled reference is
the oracle's answer on them, every reference output is a finite fp32 number, almost no row is too small to be measured, the
exponents really vary inside a tile, and the containment sets are what the containment test needs."""
import numpy as np
import pytest

import _dynamic_range_cases as drc

COMBOS = [(lay, g) for lay in drc.LAYOUTS for g in drc.GLOBALS]


def test_rowwise_err_is_the_one_shared_measure():
    ref = np.array([[1.0, 2.0], [0.0, 0.0], [1e-20, 0.0]])
    assert drc.rowwise_err(ref * [[1.0], [1.0], [1.5]], ref) == pytest.approx(0.5)
    with pytest.raises(AssertionError):
        drc.rowwise_err(ref + [[0.0], [1e-30], [0.0]], ref)          # a zero row must come out as zeros
    import test_gpu_parity
    assert test_gpu_parity.rowwise_err is drc.rowwise_err           # imported there, not forked


@pytest.mark.parametrize('name', sorted(drc.SHAPES))
@pytest.mark.parametrize('layout', drc.LAYOUTS + tuple(drc.PERTURBED_LAYOUTS))
def test_scaled_inputs_are_exact_and_the_base_problem_has_its_edge_cases(name, layout):
    N, k, I, O, B, R = drc.SHAPES[name]
    edges, sten, no_out, no_in = drc.mesh(name)
    assert np.bincount(edges[:, 0], minlength=N)[no_out] == 0 and np.bincount(edges[:, 1], minlength=N)[no_in] == 0
    x0, gy0, W0, params = drc.base(name)
    assert not x0[drc.ZERO_X_ROW].any() and not W0[drc.ZERO_W_ROW].any() and not W0[:, drc.ZERO_W_COL].any()
    assert (x0 == 0).sum() > I                                      # exact zeros beyond the zero row
    a, d, b, c = drc.exponents(name, layout)
    base_layout = drc.PERTURBED_LAYOUTS.get(layout, layout)
    a0, d0 = drc.exponents(name, base_layout)[:2]
    for rng, e in ((drc.A_RANGE, a0), (drc.D_RANGE, d0), (drc.B_RANGE, b), (drc.C_RANGE, c)):
        assert e.min() == rng[0] and e.max() == rng[1]
    for gname, (gX, gG) in drc.GLOBALS.items():
        if layout in drc.PERTURBED_LAYOUTS and gname != 'unit-unit':
            continue
        x, gy, W = drc.scaled_inputs(name, layout, gX, gG)
        for t, t0, f in ((x, x0, np.ldexp(1.0, a + gX)[:, None]), (gy, gy0, np.ldexp(1.0, d + gG)[:, None]),
                         (W, W0, np.ldexp(1.0, b[:, None] + c[None, :])[:, :, None, None])):
            assert t.dtype == np.complex64 and np.isfinite(t.view(np.float32)).all()
            assert np.array_equal(t.astype(np.complex128), t0.astype(np.complex128) * f)        # powers of two, nothing rounded
        box = (np.abs(x.real) < 1e-7) & (np.abs(x.imag) < 1e-7)
        if drc.regime_of(gX) == 'lin':
            assert box.all()
        else:       # the exact zeros and the planted entries only -- and those well inside, the others well outside the box
            assert box.sum() == (x0 == 0).sum() + 3 * drc.special_rows(name).size
            assert np.maximum(np.abs(x.real), np.abs(x.imag))[box].max() < 0.7e-7
            assert np.maximum(np.abs(x.real), np.abs(x.imag))[~box].min() > 1.15e-7
    for ftype in (0, 1, 2):
        z, s, p = drc.scaled_params(name, base_layout, ftype)
        z0, s0, p0 = params[ftype]
        assert z.dtype == s.dtype == np.float32 and z.shape == z0.shape and s.shape == s0.shape and p is p0
        f = np.ldexp(1.0, b[:, None] + c[None, :])
        assert np.array_equal(z.astype(np.float64), z0 * f.reshape(f.shape + (1,) * (z0.ndim - 2)))
        assert np.array_equal(s.astype(np.float64), s0 * f.reshape(f.shape + (1,) * (s0.ndim - 2)))


@pytest.mark.parametrize('name', sorted(drc.SHAPES))
def test_every_tile_of_the_random_layout_spans_the_exponent_range(name):
    N = drc.SHAPES[name][0]
    a, d, _, _ = drc.exponents(name, 'random')
    for t in range((N + drc.TILE - 1) // drc.TILE):
        at = a[t * drc.TILE:(t + 1) * drc.TILE]
        assert at.max() - at.min() >= 10, (t, at)
    # ... and the tile-coherent layout is constant on a tile (the rows pinned for the planted entries aside), alternating from tile to tile
    a, d, _, _ = drc.exponents(name, 'tiles')
    pinned = np.zeros(N, bool)
    pinned[drc.special_rows(name)] = True
    first = a[::drc.TILE]
    assert all(np.all(a[t * drc.TILE:(t + 1) * drc.TILE][~pinned[t * drc.TILE:(t + 1) * drc.TILE]] == first[t]) for t in range(first.size) if not pinned[t * drc.TILE])
    assert np.all(np.abs(np.diff(first[[not pinned[t * drc.TILE] for t in range(first.size)]])) == drc.A_RANGE[1] - drc.A_RANGE[0])
    assert set(zip(a[~pinned].tolist(), d[~pinned].tolist())) == {(x, y) for x in drc.A_RANGE for y in drc.D_RANGE}


@pytest.mark.parametrize('layout,gname', COMBOS, ids=['%s-%s' % c for c in COMBOS])
def test_rescaled_reference_is_the_oracle_on_the_scaled_inputs(layout, gname):
    """At the smallest shape: every layout and every pair of global exponents, both regimes of the origin box."""
    gX, gG = drc.GLOBALS[gname]
    ref = drc.scaled_reference(drc.SMALLEST, layout, gX, gG)
    direct = drc.direct_reference(drc.SMALLEST, layout, gX, gG)
    for r, dct in zip(ref, direct):
        assert drc.rowwise_err(r, dct) < 1e-12


@pytest.mark.parametrize('layout', tuple(drc.PERTURBED_LAYOUTS))
def test_rescaled_reference_of_the_perturbed_layouts(layout):
    ref = drc.scaled_reference(drc.SMALLEST, layout, 0, 0)
    direct = drc.direct_reference(drc.SMALLEST, layout, 0, 0)
    for r, dct in zip(ref, direct):
        assert drc.rowwise_err(r, dct) < 1e-12


@pytest.mark.parametrize('name', sorted(drc.SHAPES))
@pytest.mark.parametrize('layout', drc.LAYOUTS)
def test_references_are_fp32_numbers_and_few_rows_are_too_small(name, layout):
    """A condition on the INPUTS: the exponent ranges are chosen so that the reference alone meets it, at every shape, layout and
    pair of global exponents the GPU tests use."""
    for gname, (gX, gG) in drc.GLOBALS.items():
        drc.assert_reference_in_range(name, layout, gX, gG, gname)


@pytest.mark.parametrize('name,ftype', drc.PARAM_CASES)
def test_parameter_path_references_are_in_range_too(name, ftype):
    for gname in drc.PARAM_GLOBALS:
        drc.assert_reference_in_range(name, 'random', *drc.GLOBALS[gname], tag=gname, wkind=ftype)


@pytest.mark.parametrize('name', drc.CONTAINMENT_SHAPES)
@pytest.mark.parametrize('layout', tuple(drc.PERTURBED_LAYOUTS))
def test_perturbed_references_are_in_range(name, layout):
    drc.assert_reference_in_range(name, layout, 0, 0)


@pytest.mark.parametrize('name', drc.STREAMING_SHAPES)
@pytest.mark.parametrize('layout', drc.LAYOUTS)
def test_tiny_cotangents_reach_the_underflow_of_the_squared_inverse_scale(name, layout):
    """The streaming gather gives row j of H = sum over j's out-edges of gy[dst] conj(S) the inverse scale 2^(E - 13), E the exponent
    of the row's largest component; its SQUARE is zero in fp32 once 2 (E - 13) < -149, i.e. the row below 2^-61.  Bounded from above
    per row by sum_e max|gy[dst_e]| max|S_e| sqrt 2: in every combination with a tiny gy EVERY row of H is below 2^-62, whatever x
    holds -- each tile's share of gW depends on a bound of the second operand that does not square that inverse scale."""
    N = drc.SHAPES[name][0]
    edges, sten = drc.mesh(name)[:2]
    smax = np.abs(sten).reshape(sten.shape[0], -1).max(axis=1).astype(np.float64)
    for gname in ('unit-tiny', 'huge-tiny', 'tiny-tiny'):
        gy = drc.scaled_inputs(name, layout, *drc.GLOBALS[gname])[1]
        gmax = np.abs(gy).max(axis=1).astype(np.float64)
        bound = np.sqrt(2.0) * np.bincount(edges[:, 0], weights=gmax[edges[:, 1]] * smax, minlength=N)
        below = bound < 2.0 ** -62
        assert below.all(), (gname, below.mean(), float(np.log2(bound.max())))


@pytest.mark.parametrize('name', drc.CONTAINMENT_SHAPES + ('stream3075',))
def test_containment_sets(name):
    N = drc.dims(name)[0]
    P = drc.perturbed_set(name)
    assert 0 < P.size <= max(1, round(0.02 * N)) and np.all(P % drc.TILE == drc.TILE - 1)
    inP = np.zeros(N, bool)
    inP[P] = True
    edges = drc.mesh(name)[0]
    for affected in drc.affected_rows(name, P):
        assert affected[P].all()                            # (every vertex has its self-edge)
        un = ~affected
        assert un.mean() >= 0.30, un.mean()
        tiles = np.arange(N) // drc.TILE
        assert any(affected[tiles == t].any() and un[tiles == t].any() for t in range(tiles.max() + 1))
        assert un[P + 1].any()                              # an unaffected row directly behind a perturbed one
    ya, ga = drc.affected_rows(name, P)
    # by definition: no unaffected y row has an in-edge from P, no unaffected gx row an out-edge into P
    assert not (inP[edges[:, 0]] & ~ya[edges[:, 1]]).any() and not (inP[edges[:, 1]] & ~ga[edges[:, 0]]).any()
