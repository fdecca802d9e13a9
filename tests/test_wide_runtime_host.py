"""Pins the cases of the wide-path and run-time-path tests (_wide_runtime_cases.py on the generator of _dynamic_range_cases.py) on
the CPU: the scaled inputs are exact, the rescaled reference is the oracle's answer on them, every reference is a finite fp32
number with almost no row too small to be measured at every pair of global exponents the GPU tests use, and the block arithmetic
those tests rely on -- block counts, tail widths, the 77-channel bound of the double-precision gather, the k split of the
filter-gradient GEMM -- is what the library's sources say."""
import numpy as np
import pytest

import _dynamic_range_cases as drc
import _wide_runtime_cases as wrc
import test_dynamic_range_host as drh

WIDE = tuple(wrc.WIDE_SHAPES) + tuple(wrc.DENSE_SHAPES)
RT = tuple(wrc.RT_SHAPES)


def layouts_of(name):
    return drc.LAYOUTS if name in WIDE else ('random',)         # (the run-time cases use the random layout only)


def globals_of(name):
    return wrc.WIDE_GLOBALS if name in WIDE else wrc.RT_GLOBALS


CASES = [(name, layout) for name in WIDE + RT for layout in layouts_of(name)]


def test_the_shapes_live_beside_the_record_shapes_and_share_the_measure():
    assert not set(wrc.SHAPES) & set(drc.SHAPES)                # the sweeps over drc.SHAPES keep their cases
    assert all(drc.dims(name) == dims for name, dims in wrc.SHAPES.items())
    assert set(wrc.WIDE_GLOBALS) | set(wrc.RT_GLOBALS) <= set(drc.GLOBALS)
    ref = np.array([[1.0, 2.0], [4.0, 0.0]])
    got = ref + [[0.5, 0.0], [0.0, 0.0]]
    assert wrc.rows_and_columns_err(got, ref) == (pytest.approx(0.25), pytest.approx(0.125))      # 0.5 / max of row 0, 0.5 / max of column 0
    import test_gpu_wide_runtime as gpu
    assert gpu.drc is drc and not hasattr(gpu, 'rowwise_err') and not hasattr(gpu, 'measured_err')      # used from there, not forked


@pytest.mark.parametrize('name,layout', CASES, ids=['%s-%s' % c for c in CASES])
def test_scaled_inputs_are_exact_and_the_base_problem_has_its_edge_cases(name, layout):
    """The check of test_dynamic_range_host.py, at the pairs of global exponents of these cases."""
    N, k, I, O, B, R = drc.dims(name)
    edges, sten, no_out, no_in = drc.mesh(name)
    assert sten.shape[1:] == (R, 2 * B + 1) and sten.dtype == np.complex64 and edges.max() < N
    assert np.bincount(edges[:, 0], minlength=N)[no_out] == 0 and np.bincount(edges[:, 1], minlength=N)[no_in] == 0
    x0, gy0, W0, params = drc.base(name)
    assert not x0[drc.ZERO_X_ROW].any() and not W0[drc.ZERO_W_ROW].any() and not W0[:, drc.ZERO_W_COL].any()
    assert (x0 == 0).sum() > I
    a, d, b, c = drc.exponents(name, layout)
    for rng, e in ((drc.A_RANGE, a), (drc.D_RANGE, d), (drc.B_RANGE, b), (drc.C_RANGE, c)):
        assert e.min() == rng[0] and e.max() == rng[1]
    for gname in globals_of(name):
        gX, gG = drc.GLOBALS[gname]
        x, gy, W = drc.scaled_inputs(name, layout, gX, gG)
        for t, t0, f in ((x, x0, np.ldexp(1.0, a + gX)[:, None]), (gy, gy0, np.ldexp(1.0, d + gG)[:, None]),
                         (W, W0, np.ldexp(1.0, b[:, None] + c[None, :])[:, :, None, None])):
            assert t.dtype == np.complex64 and np.isfinite(t.view(np.float32)).all()
            assert np.array_equal(t.astype(np.complex128), t0.astype(np.complex128) * f)
        box = (np.abs(x.real) < 1e-7) & (np.abs(x.imag) < 1e-7)
        if drc.regime_of(gX) == 'lin':
            assert box.all()
        else:
            assert box.sum() == (x0 == 0).sum() + 3 * drc.special_rows(name).size
            assert np.maximum(np.abs(x.real), np.abs(x.imag))[box].max() < 0.7e-7
            assert np.maximum(np.abs(x.real), np.abs(x.imag))[~box].min() > 1.15e-7
    for ftype in (0, 1, 2):
        z, s, p = drc.scaled_params(name, layout, ftype)
        z0, s0, p0 = params[ftype]
        f = np.ldexp(1.0, b[:, None] + c[None, :])
        assert z.dtype == s.dtype == np.float32 and p is p0
        assert np.array_equal(z.astype(np.float64), z0 * f.reshape(f.shape + (1,) * (z0.ndim - 2)))
        assert np.array_equal(s.astype(np.float64), s0 * f.reshape(f.shape + (1,) * (s0.ndim - 2)))


def test_the_dense_rows_of_wide129_do_not_factor():
    """FCPrecomp's stencil is rank one with two adjacent rings; the random one is neither, so the graph build keeps dense rows."""
    sten = drc.mesh('wide129dense')[1]
    assert (np.abs(sten) > 0).all()                                           # all three rings carry weight
    assert (np.linalg.matrix_rank(sten.astype(np.complex128)) == 3).all()        # (E, R, F) = (E, 3, 3): full rank, not w[r] ph[f]
    fc = drc.mesh('wide129')[1]
    assert (np.linalg.matrix_rank(fc.astype(np.complex128), tol=1e-5) <= 1).all()
    x, xd = drc.base('wide129')[0], drc.base('wide129dense')[0]
    assert np.array_equal(x, xd)                                              # the same features and filter on either stencil


@pytest.mark.parametrize('name', WIDE + RT)
def test_rescaled_reference_is_the_oracle_on_the_scaled_inputs(name):
    for layout in layouts_of(name):
        for gname in globals_of(name):
            gX, gG = drc.GLOBALS[gname]
            ref = drc.scaled_reference(name, layout, gX, gG)
            direct = drc.direct_reference(name, layout, gX, gG)
            for r, dct in zip(ref, direct):
                assert drc.rowwise_err(r, dct) < 1e-12, (layout, gname)


@pytest.mark.parametrize('name,layout', CASES, ids=['%s-%s' % c for c in CASES])
def test_references_are_fp32_numbers_and_few_rows_are_too_small(name, layout):
    """A condition on the INPUTS (drc.MAX_EXCLUDED is a cap, not a measurement), at every pair the GPU tests use."""
    for gname in globals_of(name):
        drc.assert_reference_in_range(name, layout, *drc.GLOBALS[gname], tag=gname)


@pytest.mark.parametrize('name,ftype', wrc.WIDE_PARAM_CASES + wrc.RT_PARAM_CASES)
def test_parameter_path_references_are_in_range_too(name, ftype):
    for gname in globals_of(name):
        drc.assert_reference_in_range(name, 'random', *drc.GLOBALS[gname], tag=gname, wkind=ftype)


def test_containment_sets_of_wide129():
    """By rows: the conditions of test_dynamic_range_host.py::test_containment_sets, and the perturbed references in range.  By
    channel blocks: input block 1 and output block 1 exist, are full blocks, and leave channels on both sides."""
    drh.test_containment_sets('wide129')
    for layout in drc.PERTURBED_LAYOUTS:
        drc.assert_reference_in_range('wide129', layout, 0, 0)
        for r, dct in zip(drc.scaled_reference('wide129', layout, 0, 0), drc.direct_reference('wide129', layout, 0, 0)):
            assert drc.rowwise_err(r, dct) < 1e-12
    x, gy, _ = drc.scaled_inputs('wide129', 'random', 0, 0)
    xp = drc.scaled_inputs('wide129', 'random+xP', 0, 0)[0]
    P = drc.perturbed_set('wide129')
    assert np.array_equal(xp[P], x[P] * np.float32(2.0 ** drc.PERTURB_EXP)) and np.isfinite(xp.view(np.float32)).all()
    N, k, I, O, B, R = drc.dims('wide129')
    assert wrc.blocks(I, wrc.MAX_BLOCK)[1] == (64, 64) and wrc.blocks(O, wrc.MAX_BLOCK)[1] == (64, 1)
    assert drc.ZERO_W_ROW < 64 and drc.ZERO_W_COL < 64                        # the zero row and column lie in the blocks that must not change


# ---------------------------------------------------------------- block arithmetic
def test_channel_blocks_and_tails():
    assert wrc.blocks(129, 64) == [(0, 64), (64, 64), (128, 1)] and wrc.blocks(65, 64) == [(0, 64), (64, 1)]
    assert wrc.blocks(128, 64) == [(0, 64), (64, 64)] and wrc.blocks(64, 64) == [(0, 64)]
    assert [w for _, w in wrc.blocks(80, 64)] == [64, 16] and [w for _, w in wrc.blocks(72, 64)] == [64, 8]
    for blk in (56, 48, 40, 32):                                # whatever block < 64 the library picks at 8 rings, 70 -> 60 channels is wide
        bi, bo = wrc.blocks(70, blk), wrc.blocks(60, blk)
        assert len(bi) >= 2 and sum(w for _, w in bi) == 70 and sum(w for _, w in bo) == 60 and all(0 < w <= blk for _, w in bi + bo)
    for name, dims in wrc.WIDE_SHAPES.items():                  # every wide case is wide at the widest block the kernels have
        assert max(dims[2], dims[3]) > wrc.MAX_BLOCK, name
    from fieldconv_amd.functional import MAX_CHANNELS
    assert MAX_CHANNELS == wrc.MAX_BLOCK
    # a one-channel block has rows of 8 bytes: every second one off the 16-byte grid
    assert (1 * 8) % 16 == 8


def test_gather_blocks_of_the_run_time_path():
    """fc_generic_gather cuts the input channels so that one workgroup's (R, F) accumulators fit into kMaxLds = 160 KiB."""
    import os
    import re
    here = os.path.dirname(os.path.abspath(__file__))
    src = open(os.path.join(here, '..', 'fieldconv_amd', 'csrc', 'fc_kernels.hpp')).read()
    m = re.search(r'constexpr size_t kMaxLds = (\d+) \* 1024;', src)
    assert m and int(m.group(1)) * 1024 == wrc.MAX_LDS
    N, k, I, O, B, R = drc.dims('rt_blocks_f64')
    F = 2 * B + 1
    assert (R, F) == (12, 11)
    assert wrc.gather_block(R, F, 16) == 77 and 78 * R * F * 16 > wrc.MAX_LDS >= 77 * R * F * 16           # complex128
    assert wrc.blocks(I, 77) == [(0, 77), (77, 3)]
    assert wrc.gather_block(R, F, 8) == 155 and wrc.blocks(I, min(I, 155)) == [(0, 80)]                    # complex64: one block
    for name in RT:                                                                                       # every other case: one block
        n_, k_, I_, O_, B_, R_ = drc.dims(name)
        if name != 'rt_blocks_f64':
            assert I_ <= wrc.gather_block(R_, 2 * B_ + 1, 16), name


def test_k_split_of_the_filter_gradient_product():
    """cgemm_ksplit restated: rt_ksplit's gW product, and the first two GEMM sizes, are cut along k on any device of 6 or more
    compute units; the other sizes are not on any device (the GPU tests assert the library's own answer, fc_cgemm_workspace_bytes,
    which needs the device's count)."""
    N, k, I, O, B, R = drc.dims('rt_ksplit')
    K = I * R * (2 * B + 1)
    assert (O, K, N) == (5, 162, 2100) == wrc.CGEMM_SIZES[0]
    for cus in (6, 64, 256, 304):
        assert wrc.cgemm_slices(O, K, N, cus) > 1 and wrc.cgemm_slices(1, 1, 2049, cus) > 1
        assert wrc.cgemm_slices(1, 1, 2047, cus) == 1                          # K < 2048
        assert wrc.cgemm_slices(65, 64, 16, cus) == 1 and wrc.cgemm_slices(70, 333, 130, cus) == 1
        assert wrc.cgemm_slices(N, O, K, cus) == 1 and wrc.cgemm_slices(N, K, O, cus) == 1       # the two other layouts of rt_ksplit
    assert wrc.cgemm_slices(5, 162, 2100, 256) == 5 and wrc.cgemm_slices(1, 1, 2049, 256) == 5    # ceil(K / 512) slices of 432 / 416


@pytest.mark.parametrize('size', wrc.CGEMM_SIZES, ids=lambda s: 'O%d_K%d_n%d' % s)
def test_cgemm_operands(size):
    """Rows scaled exactly; every product an fp32 number; and the products are well conditioned row by row and column by column:
    numpy's own complex64 product stays under a quarter of the complex64 gate (1e-5)."""
    c = wrc.cgemm_case(*size)
    for t, t0, e, rng in ((c['A'], c['A0'], c['a'], wrc.CGEMM_A_RANGE), (c['G'], c['G0'], c['d'], wrc.CGEMM_G_RANGE)):
        assert e.min() == rng[0] and e.max() == rng[1]
        assert np.array_equal(t.astype(np.complex128), t0.astype(np.complex128) * np.ldexp(1.0, e)[:, None])
    A, W, G = c['A'], c['W'], c['G']
    low = {'y': A @ W.T * np.float32(0.5), 'gC': G @ W.conj(), 'gW': G.T @ A.conj() * np.float32(2.0)}
    for key, ref in c['ref'].items():
        assert np.isfinite(ref.astype(np.complex64).view(np.float32)).all()
        assert (drc.row_max(ref) > 2.0 ** drc.FLOOR_EXP).all() and (drc.row_max(ref.T) > 2.0 ** drc.FLOOR_EXP).all()
        er, ec = wrc.rows_and_columns_err(low[key], ref)
        assert er < 2.5e-6 and ec < 2.5e-6, (key, er, ec)
