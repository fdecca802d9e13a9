"""Host-side checks of the level-transfer feature (fieldconv_amd.transfer, csrc/fc_transfer.hip): the numpy restatement against a
dense matrix product, the pool weights, argument validation (everything is rejected before a device is needed) and the C ABI
surface.  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _transfer_ref as tref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize('complex_x', [True, False])
@pytest.mark.parametrize('conj', [False, True])
def test_restatement_equals_a_dense_product(complex_x, conj):
    rows, weight, phase, empty = tref.random_plan()
    x = tref.features(300, 5, complex_x, 3)
    g = tref.features(40, 5, complex_x, 4)
    T = tref.dense(rows, weight, phase, conj, 40, 300, complex_x)
    y64 = tref.transfer(rows, weight, phase, conj, 40, x, np.float64)
    assert np.abs(y64 - T @ x).max() <= 1e-12 * np.abs(T @ x).max()
    assert np.all(y64[empty] == 0) and np.count_nonzero(np.abs(y64).sum(1)) == 40 - len(empty)
    gx64 = tref.adjoint(rows, weight, phase, conj, 300, g, np.float64)
    assert np.abs(gx64 - T.conj().T @ g).max() <= 1e-12 * np.abs(T.conj().T @ g).max()
    y32 = tref.transfer(rows, weight, phase, conj, 40, x, np.float32)
    assert y32.dtype == (np.complex64 if complex_x else np.float32)
    assert 0 < np.abs(y32 - y64).max() <= 1e-4 * np.abs(y64).max()
    # the long row and the duplicates are there
    counts = np.bincount(rows[:, 0], minlength=40)
    assert counts.max() == 200 and len(np.unique(rows, axis=0)) < len(rows) and np.any(np.diff(rows[:, 0]) < 0)


def test_one_slot_plan_has_one_slot_per_row():
    rows, weight, phase = tref.one_slot_plan()
    assert np.array_equal(np.sort(rows[:, 0]), np.arange(300)) and rows[:, 1].max() < 40


def test_pool_weights_of_every_non_empty_cell_sum_to_one():
    rng = np.random.default_rng(0)
    S_c = 17
    cell = rng.integers(-1, S_c, 400)
    cell[cell == 5] = 6                                   # an empty cell
    w = rng.random(400).astype(np.float32)
    w[cell == 9] = 0                                      # a cell without mass: 1 / n_c
    member, c, weight = tref.pool_weights(cell, w, S_c)
    assert np.array_equal(member, np.nonzero(cell >= 0)[0]) and weight.dtype == np.float32
    sums = np.bincount(c, weights=weight.astype(np.float64), minlength=S_c)
    filled = np.bincount(c, minlength=S_c) > 0
    assert not filled[5] and filled.sum() == S_c - 1
    assert np.abs(sums[filled] - 1).max() <= 1e-6
    assert np.all(weight[c == 9] == np.float32(1) / np.float32((cell == 9).sum()))


def _plan_args():
    rows = torch.tensor([[0, 1], [2, 0], [1, 1]], dtype=torch.int64)
    return rows, torch.ones(3), torch.ones(3, dtype=torch.complex64)


@pytest.mark.parametrize('change', ['out high', 'in high', 'negative', 'rows dtype', 'rows shape', 'weight dtype', 'phase dtype',
                                    'weight length', 'phase length', 'no sizes', 'conj'])
def test_transfer_plan_rejects_bad_arguments(change):
    from fieldconv_amd.transfer import TransferPlan
    rows, weight, phase = _plan_args()
    kw = dict(n_out=3, n_in=2)
    if change == 'out high':
        kw['n_out'] = 2
    elif change == 'in high':
        kw['n_in'] = 1
    elif change == 'negative':
        rows = rows.clone()
        rows[1, 1] = -1
    elif change == 'rows dtype':
        rows = rows.to(torch.int32)
    elif change == 'rows shape':
        rows = rows.t().contiguous()
    elif change == 'weight dtype':
        weight = weight.to(torch.float16)
    elif change == 'phase dtype':
        phase = torch.ones(3)
    elif change == 'weight length':
        weight = torch.ones(4)
    elif change == 'phase length':
        phase = torch.ones(2, dtype=torch.complex64)
    elif change == 'no sizes':
        kw = dict(n_out=3)
    elif change == 'conj':
        kw['conj_phase'] = 1
    with pytest.raises(ValueError):
        TransferPlan(rows, weight, phase, **kw)


def test_a_non_ascending_coarse_is_rejected():
    from fieldconv_amd.transfer import level_transfer, sample_cells
    pos, face = tref.flat_grid(4)
    pos, face = torch.from_numpy(pos), torch.from_numpy(face)
    samples = torch.arange(16)
    for coarse in (torch.tensor([3, 1]), torch.tensor([2, 2]), torch.tensor([0, 16]), torch.tensor([1, 2], dtype=torch.int32)):
        with pytest.raises(ValueError):
            sample_cells(pos, face, samples, coarse)
        with pytest.raises(ValueError):
            level_transfer(pos, face, samples, coarse, torch.ones(16))
    with pytest.raises(ValueError):          # the range tables of a batch go together
        sample_cells(pos, face, samples, torch.tensor([0, 5]), pos_ptr=torch.tensor([0, 16]))


def test_tangent_transfer_has_no_cpu_path():
    from fieldconv_amd.transfer import TransferPlan, tangent_transfer
    plan = TransferPlan.__new__(TransferPlan)._set(None, None, 3, 2, 0, False, torch.device('cpu'))
    with pytest.raises(RuntimeError):
        tangent_transfer(torch.zeros(2, 4, dtype=torch.complex64), plan)
    with pytest.raises(TypeError):
        tangent_transfer(torch.zeros(2, 4, dtype=torch.float16), plan)
    with pytest.raises(ValueError):
        tangent_transfer(torch.zeros(2, 4), None)


def test_header_binding_and_library_export_the_new_symbol():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert 'fc_transfer' in declared and 'fc_transfer' in _lib.SIGNATURES and 'fc_transfer.hip' in build.SOURCES
    assert len(_lib.SIGNATURES['fc_transfer'][1]) == 14
    lib = ctypes.CDLL(build.build_native())
    assert hasattr(lib, 'fc_transfer') and _lib.load().fc_abi_version() == 11


def test_public_names():
    from fieldconv_amd import functional, nn, transfer, transforms
    for name in ('TransferPlan', 'tangent_transfer', 'sample_cells', 'level_transfer'):
        assert getattr(functional, name) is getattr(transfer, name)
    assert 'CoarsenSamples' in transforms.__all__ and {'TangentPool', 'TangentUnpool'} <= set(nn.__all__)
    assert not list(nn.TangentPool().parameters()) and not nn.TangentUnpool().state_dict()
