"""Host-side checks of max pooling by magnitude (fieldconv_amd.transfer.tangent_transfer_max, fieldconv_amd.pooling.mesh_max,
csrc/fc_maxpool.hip): the numpy restatement tests/_maxpool_ref.py against a brute-force loop, the tie rule, the independence of the
(key, slot) order from how the candidates are split, the C ABI surface and the argument checks.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _maxpool_ref as mref
import _transfer_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {'fc_transfer_max', 'fc_transfer_max_backward', 'fc_segment_max_forward', 'fc_segment_max_backward'}


def tiny_plan():
    """6 outputs, 20 inputs: row 4 is empty, the pair [1, 7] is listed twice with two different phases, rows given unsorted"""
    rng = np.random.default_rng(3)
    out = np.array([0, 0, 0, 1, 1, 1, 1, 2, 2, 3, 3, 3, 3, 3, 5, 5, 0, 2, 1, 5])
    inn = np.array([2, 9, 13, 7, 4, 7, 18, 0, 11, 5, 6, 15, 19, 3, 8, 17, 1, 12, 10, 14])
    rows = np.stack((out, inn), 1)[rng.permutation(20)].astype(np.int64)
    assert (rows == [1, 7]).all(1).sum() == 2 and 4 not in rows[:, 0]
    phase = np.exp(1j * rng.uniform(-np.pi, np.pi, 20)).astype(np.complex64)
    return rows, phase


def brute_force(rows, phase, conj, n_out, x, real):
    """(arg, y) by the definition, one scalar at a time"""
    order = np.argsort(rows[:, 0], kind='stable')
    r, ph = rows[order], phase[order]
    C = x.shape[1]
    arg = np.full((n_out, C), -1, dtype=np.int64)
    y = np.zeros((n_out, C), dtype=x.dtype)
    for o in range(n_out):
        for c in range(C):
            best = None
            for e in range(len(r)):
                if r[e, 0] != o:
                    continue
                v = x[r[e, 1], c]
                if np.iscomplexobj(x):
                    re, im = real(v.real), real(v.imag)
                    k = real(real(re * re) + real(im * im))
                else:
                    k = real(v)
                if best is None or k > best[0] or (k == best[0] and e < best[1]):
                    best = (k, e)
            if best is not None:
                e = best[1]
                arg[o, c] = e
                u = np.conj(ph[e]) if conj else ph[e]
                y[o, c] = u.astype(x.dtype) * x[r[e, 1], c] if np.iscomplexobj(x) else x[r[e, 1], c]
    return arg, y


@pytest.mark.parametrize('complex_x', [True, False])
@pytest.mark.parametrize('conj', [False, True])
def test_restatement_equals_a_brute_force_loop(complex_x, conj):
    rows, phase = tiny_plan()
    x = tref.features(20, 3, complex_x, 5).astype(np.complex64 if complex_x else np.float32)
    x = mref.plant_ties(rows, 6, x, every=1)
    assert mref.top_ties(rows, 6, x, np.float32) >= 2
    arg, y = brute_force(rows, phase, conj, 6, x, np.float32)
    got = mref.transfer_winners(rows, 6, x, np.float32)
    assert np.array_equal(got, arg) and np.all(arg[4] == -1) and np.all(np.delete(arg, 4, 0) >= 0)
    y32 = mref.transfer_forward(rows, phase, conj, x, got, np.float32)
    assert y32.dtype == x.dtype and np.all(y32[4] == 0)
    assert np.array_equal(y32.view(np.uint32), y.view(np.uint32)) if not complex_x else np.abs(y32 - y).max() <= 1e-6 * np.abs(y).max()
    y64 = mref.transfer_forward(rows, phase, conj, x, got, np.float64)
    assert np.abs(y64 - y).max() <= 1e-6 * np.abs(y).max()
    if complex_x:          # the magnitude of the output is the largest magnitude of the row
        r = rows[tref.grouped(rows)]
        for o in (0, 1, 2, 3, 5):
            assert np.allclose(np.abs(y64[o]), np.abs(x[r[r[:, 0] == o, 1]]).max(0), rtol=1e-6)
    # the gradient: <gy, dy> for a perturbation of the winners only, and exactly zero everywhere else
    gy = tref.features(6, 3, complex_x, 6).astype(x.dtype)
    gx = mref.transfer_backward(rows, phase, conj, 20, gy, got, np.float64)
    won = np.zeros((20, 3), dtype=bool)
    won[mref.winner_rows(rows, got)[got >= 0], np.nonzero(got >= 0)[1]] = True
    assert np.all(gx[~won] == 0) and np.all(gx[won] != 0)
    dx = tref.features(20, 3, complex_x, 7) * 1e-9
    dy = mref.transfer_forward(rows, phase, conj, x + dx, got, np.float64) - y64
    lhs, rhs = np.sum(np.real(np.conj(gy) * dy)), np.sum(np.real(np.conj(gx) * dx))
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)


def test_the_tie_rule_is_the_smallest_slot():
    """the duplicated pair [1, 7]: both slots hold the same entry, the earlier slot wins and its phase is the one applied; -x and
    i x tie with x exactly; -0.0 and +0.0 tie as real keys and the earlier slot's bits come out"""
    rows, phase = tiny_plan()
    r = rows[tref.grouped(rows)]
    x = tref.features(20, 2, True, 8).astype(np.complex64)
    x[7] = 50                                              # the largest entry of row 1, twice a member
    arg = mref.transfer_winners(rows, 6, x, np.float32)
    first, second = np.nonzero((r == [1, 7]).all(1))[0]
    assert first < second and np.all(arg[1] == first)
    y = mref.transfer_forward(rows, phase, False, x, arg, np.float64)
    ph = phase[tref.grouped(rows)]
    assert ph[first] != ph[second] and np.allclose(y[1], 50 * ph[first].astype(np.complex128))
    z = np.complex64(0.3 - 1.7j)
    for other in (-z, z * 1j, np.conj(z) * 1j):
        assert mref.key(np.array([other]), np.float32)[0] == mref.key(np.array([z]), np.float32)[0]
    assert mref.combine([(np.float32(2), 5), (np.float32(2), 3), (np.float32(1), 0)]) == (np.float32(2), 3)
    assert mref.combine([(np.float32(-0.0), 4), (np.float32(0.0), 9)])[1] == 4 and mref.combine([]) == (None, -1)
    xr = -np.abs(tref.features(20, 1, False, 9)).astype(np.float32) - 1
    members = r[r[:, 0] == 3, 1]
    xr[members[1], 0], xr[members[3], 0] = -0.0, 0.0
    argr = mref.transfer_winners(rows, 6, xr, np.float32)
    yr = mref.transfer_forward(rows, None, False, xr, argr, np.float32)
    assert r[argr[3, 0], 1] == members[1] and np.signbit(yr[3, 0]) and yr[3, 0] == 0


def test_the_order_does_not_depend_on_the_split():
    """an argmax over random splits of the candidates, combined by (key, slot), equals the plain argmax -- with ties present"""
    rng = np.random.default_rng(11)
    for trial in range(50):
        n = int(rng.integers(1, 400))
        k = rng.integers(0, 6, n).astype(np.float32)            # few distinct keys: many ties
        plain = int(np.argmax(k))
        cuts = np.sort(rng.integers(0, n + 1, int(rng.integers(0, 9))))
        parts = [p for p in np.split(rng.permutation(n) if trial % 2 else np.arange(n), cuts)]
        partial = [mref.combine([(k[s], int(s)) for s in part]) for part in parts]
        rng.shuffle(partial)
        assert mref.combine([p for p in partial if p[1] >= 0])[1] == plain
    x, ptr = mref.mesh_case(5, True)
    plain = mref.mesh_winners(x, ptr, np.float32)
    for chunk in (1, 7, 64, 5000):
        assert np.array_equal(mref.mesh_winners(x, ptr, np.float32, chunk), plain)
    assert np.all(plain[0] == -1) and np.all(plain[1] == 0)


def test_mesh_case_has_ties_and_origin_box_entries():
    for complex_x in (True, False):
        x, ptr = mref.mesh_case(5, complex_x)
        k = mref.key(x, np.float32)
        idx = mref.mesh_winners(x, ptr, np.float32)
        tied = sum(int(((k[ptr[b]:ptr[b + 1]] == k[idx[b], np.arange(5)]).sum(0) > 1).sum()) for b in range(2, 7))
        assert tied >= 20
        out = mref.mesh_forward(x, idx, np.float32)
        assert np.all(out[0] == 0) and out.dtype == np.float32
        if complex_x:
            assert np.all(mref.origin(x[idx[2], np.arange(5)])) and np.all(out[2] == 0)          # the winner of the mesh of 63 rows is inside
            assert mref.origin(x).sum() > 100 and np.all(out[3:] > 0)
            g = np.ones((7, 5), dtype=np.float32)
            gx = mref.mesh_backward(x, idx, g, np.float64)
            assert np.count_nonzero(gx) == 5 * 5 and np.allclose(np.abs(gx[np.abs(gx) > 0]), 1)   # meshes 1, 3, 4, 5, 6: unit vectors
        else:
            assert idx[3, 0] == ptr[3] + 5 and np.signbit(out[3, 0])


def test_header_binding_and_library_export_the_new_symbols():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES) and 'fc_maxpool.hip' in build.SOURCES
    assert [len(_lib.SIGNATURES[n][1]) for n in sorted(SYMBOLS)] == [11, 12, 14, 15]
    lib = ctypes.CDLL(build.build_native())
    assert all(hasattr(lib, n) for n in SYMBOLS) and _lib.load().fc_abi_version() == 11
    for word in ('fl(fl(re * re) + fl(im * im))', 'ties go to the smallest s', 'k_new == k_old and s_new < s_old'):
        assert word in header


def test_native_entry_points_reject_bad_arguments_before_any_launch():
    """FC_ERR_BAD_ARGUMENT for sizes, dtypes and NULL buffers; an empty problem is FC_OK without a device"""
    from fieldconv_amd import _lib
    lib = _lib.load()
    one = ctypes.c_void_p(16)          # never dereferenced: every call below returns before a launch
    assert lib.fc_transfer_max(None, None, None, None, 0, 0, 5, 0, 4, 0, 1, None, None, None) == 0
    assert lib.fc_transfer_max_backward(None, None, None, None, None, None, 0, 5, 0, 0, 4, 0, 1, None, None) == 0
    for bad in (dict(C=0), dict(dtype=2), dict(cplx=2), dict(conj=2), dict(n_out=-1), dict(y=None), dict(arg=None), dict(rowptr=None)):
        a = dict(C=4, dtype=0, cplx=1, conj=0, n_out=3, y=one, arg=one, rowptr=one)
        a.update(bad)
        assert lib.fc_transfer_max(one, a['rowptr'], one, one, a['conj'], a['n_out'], 5, 7, a['C'], a['dtype'], a['cplx'], a['y'], a['arg'], None) != 0
    assert lib.fc_transfer_max_backward(one, one, one, one, None, one, 0, 3, 5, 7, 4, 0, 1, one, None) != 0          # no slot_t
    assert lib.fc_segment_max_forward(one, one, 10, 0, 4, 0, 1, one, one, one, one, None) != 0                       # B = 0
    assert lib.fc_segment_max_forward(one, one, 10, 1, 64 * 65535 + 1, 0, 1, one, one, one, one, None) != 0
    assert lib.fc_segment_max_forward(one, one, 10, 1, 4, 0, 1, one, one, None, one, None) != 0                      # no partial buffer
    assert lib.fc_segment_max_forward(one, one, 2 ** 31 - 100, 2, 4, 0, 1, one, one, one, one, None) != 0            # N + 64 B
    assert lib.fc_segment_max_backward(None, one, one, one, 10, 1, 4, 0, 1, one, None) != 0                          # complex needs x
    assert lib.fc_segment_max_backward(None, one, one, one, 0, 1, 4, 0, 0, None, None) == 0                          # nothing to do


def test_tangent_transfer_max_checks_its_arguments_before_any_launch():
    from fieldconv_amd.transfer import TransferPlan, tangent_transfer_max
    plan = TransferPlan.__new__(TransferPlan)._set(None, None, 3, 2, 0, False, torch.device('cpu'))
    with pytest.raises(RuntimeError):
        tangent_transfer_max(torch.zeros(2, 4, dtype=torch.complex64), plan)
    with pytest.raises(TypeError):
        tangent_transfer_max(torch.zeros(2, 4, dtype=torch.float16), plan)
    with pytest.raises(ValueError):
        tangent_transfer_max(torch.zeros(2, 4), None)
    with pytest.raises(ValueError):
        tangent_transfer_max(torch.zeros(2, 4, 1), plan)


def test_mesh_max_checks_its_arguments_before_any_launch():
    from fieldconv_amd.nn import MeshMaxPool, MeshPool
    from fieldconv_amd.pooling import mesh_max
    x = torch.zeros(10, 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError):
        mesh_max(x, torch.tensor([0, 4, 10]))
    with pytest.raises(RuntimeError):
        MeshMaxPool()(x, torch.tensor([0, 4, 10]))
    with pytest.raises(ValueError):
        mesh_max(torch.zeros(10, 4), torch.tensor([0, 10]))                      # real input needs soft_abs=False
    with pytest.raises(ValueError):
        mesh_max(x, torch.tensor([0, 10]), soft_abs=False)                       # complex input has the one mode
    with pytest.raises(ValueError):
        mesh_max(x[:, 0], torch.tensor([0, 10]))
    with pytest.raises(ValueError):
        mesh_max(x, torch.tensor([0, 10]), return_indices=1)
    with pytest.raises(ValueError):
        MeshPool(reduce='max')                                                   # MeshPool stays as it is


def test_public_names():
    from fieldconv_amd import functional, nn, pooling, transfer
    assert functional.tangent_transfer_max is transfer.tangent_transfer_max and functional.mesh_max is pooling.mesh_max
    assert {'TangentMaxPool', 'MeshMaxPool'} <= set(nn.__all__)
    assert not list(nn.TangentMaxPool().parameters()) and not nn.TangentMaxPool().state_dict() and not nn.MeshMaxPool().state_dict()
    assert nn.MeshMaxPool(soft_abs=False).soft_abs is False and 'soft_abs=True' in repr(nn.MeshMaxPool())
