"""Host-side checks of the counter-based generator and its two users (fieldconv_amd.dropout, fieldconv_amd.augment,
csrc/fc_philox.hpp, fc_dropout.hip, fc_augment.hip): the numpy restatement against the published known-answer vectors of
Philox4x32-10, the statistics of the restated masks, the C ABI surface, the public names, the modules' state and argument validation
(everything is rejected before a device is needed).  No GPU."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _philox_ref as pref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = {'fc_philox_words', 'fc_dropout', 'fc_mesh_affine_draw', 'fc_mesh_affine_apply'}
SEED = 2024


@pytest.mark.parametrize('case', range(len(pref.KNOWN_ANSWERS)))
def test_restatement_gives_the_published_known_answers(case):
    counter, key, expected = pref.KNOWN_ANSWERS[case]
    got = pref.philox4x32_10(counter, key)
    assert got.shape == (1, 4) and [int(w) for w in got[0]] == list(expected)


def test_restated_words_follow_the_counter_and_key_layout():
    # the third vector through the package's layout: q = (c1 << 32) | c0, hi = (c3 << 32) | c2, seed = (k1 << 32) | k0
    counter, key, expected = pref.KNOWN_ANSWERS[2]
    q, hi, seed = counter[1] << 32 | counter[0], counter[3] << 32 | counter[2], key[1] << 32 | key[0]
    assert [int(w) for w in pref.words(seed, hi, q, 1)[0]] == list(expected)
    assert [int(w) for w in pref.draw_blocks(seed, q, counter[2], counter[3])[0]] == list(expected)
    # the carry of the block number goes into the counter's second word, and wraps at 2^64
    w = pref.words(7, 9, 2 ** 32 - 2, 4)
    assert np.array_equal(w[2], pref.philox4x32_10((0, 1, 9, 0), (7, 0))[0]) and np.array_equal(w[1], pref.philox4x32_10((2 ** 32 - 1, 0, 9, 0), (7, 0))[0])
    assert np.array_equal(pref.words(7, 9, 2 ** 64 - 1, 2)[1], pref.philox4x32_10((0, 0, 9, 0), (7, 0))[0])
    # entry e is word e & 3 of block e >> 2
    e = np.array([0, 3, 4, 35, 2 ** 33 + 5], dtype=np.uint64)
    for ei, b in zip(e.tolist(), pref.bits24(SEED, 3, 1, e).tolist()):
        assert b == int(pref.draw_blocks(SEED, ei >> 2, 3, 1)[0, ei & 3]) >> 8


@pytest.mark.parametrize('p', [0.1, 0.5, 0.9])
@pytest.mark.parametrize('step', [0, 1, 2])
def test_drop_fraction_is_binomial(p, step):
    n = 4096
    keep = pref.element_keep(64, 64, p, SEED, step)
    dropped = n - int(keep.sum())
    sd = np.sqrt(n * p * (1 - p))
    print(f'p={p} step={step}: dropped {dropped} of {n}, {(dropped - n * p) / sd:+.2f} standard deviations')
    assert abs(dropped - n * p) <= 6 * sd


def test_two_steps_give_different_masks():
    a, b = pref.element_keep(64, 64, 0.5, SEED, 0), pref.element_keep(64, 64, 0.5, SEED, 1)
    differ = int((a != b).sum())
    # independent fair decisions differ with probability 1/2: 4 096 entries, standard deviation 32
    assert abs(differ - 2048) <= 6 * 32
    c = pref.channel_keep([0, 3, 3, 7], 5, 0.5, SEED, 0)
    assert c.shape == (7, 5) and (c[:3] == c[0]).all() and (c[3:] == c[3]).all()
    assert not np.array_equal(pref.channel_keep([0, 3, 3, 7], 64, 0.5, SEED, 0)[0], pref.element_keep(1, 64, 0.5, SEED, 0)[0])          # streams differ


def test_restated_values():
    x = (np.arange(12, dtype=np.float32).reshape(4, 3) - 5) * (1 + 0.5j)
    x = x.astype(np.complex64)
    keep = pref.element_keep(4, 3, 0.5, SEED, 0)
    y = pref.dropout(x, keep, 0.5)
    assert y.dtype == np.complex64 and np.array_equal(y[keep], 2 * x[keep]) and not y[~keep].any()
    assert not np.signbit(y[~keep].real).any() and not np.signbit(y[~keep].imag).any()
    assert np.array_equal(pref.dropout(x, pref.element_keep(4, 3, 0.0, SEED, 0), 0.0).view(np.uint32), x.view(np.uint32))          # p = 0: x's bits
    assert pref.threshold(0.5) == 1 << 23 and pref.threshold(0.0) == 0 and pref.threshold(0.1) == 1677721


def test_restated_augmentation():
    params = pref.affine_params(5, SEED, 1, (0.85, 1.15), (45, 30, 15))
    assert params.dtype == np.float32 and (params[:, 0] >= 0.85).all() and (params[:, 0] <= 1.15).all()
    assert (np.abs(params[:, 1:]) <= np.array([45, 30, 15])).all() and len(set(params[:, 1].tolist())) == 5
    assert (pref.affine_params(5, SEED, 1)[:, 0] == 1).all() and np.array_equal(pref.affine_params(5, SEED, 1)[:, 1:], pref.affine_params(5, SEED, 1, (1, 2))[:, 1:])
    M = pref.affine_matrix(params, np.float64)
    for b in range(5):
        R = M[b] / params[b, 0]
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12
    assert np.abs(pref.affine_matrix(params, np.float32) - M).max() <= 1e-6
    # a quarter turn about axis 2 takes e_x to e_y: right-handed, column vectors
    quarter = pref.affine_matrix(np.array([[1, 0, 0, 90]], dtype=np.float32), np.float64)[0]
    assert np.abs(quarter @ np.array([1.0, 0, 0]) - np.array([0, 1.0, 0])).max() <= 1e-7
    pos = np.arange(42, dtype=np.float32).reshape(14, 3)
    out = pref.affine_apply(pos, [0, 1, 5, 14], M.astype(np.float32)[:3], index=np.array([13, 0, 4, 14, -1]))
    assert np.isnan(out[3:]).all() and np.abs(out[0] - M[2] @ pos[13]).max() <= 1e-4 and np.abs(out[2] - M[1] @ pos[4]).max() <= 1e-4


# ------------------------------------------------------------------ the C ABI surface and the public names
def test_header_binding_and_library_export_the_new_symbols():
    from fieldconv_amd import _lib, build
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    assert SYMBOLS <= declared and SYMBOLS <= set(_lib.SIGNATURES)
    assert {'fc_dropout.hip', 'fc_augment.hip'} <= set(build.SOURCES) and 'fc_philox.hpp' in build.HEADERS
    assert [len(_lib.SIGNATURES[n][1]) for n in sorted(SYMBOLS)] == [15, 10, 13, 6]
    assert not any(n.endswith('workspace_bytes') and ('dropout' in n or 'affine' in n or 'philox' in n) for n in declared)
    lib = ctypes.CDLL(build.build_native())
    assert all(hasattr(lib, n) for n in SYMBOLS) and _lib.load().fc_abi_version() == 11


def test_bad_dims_are_refused_before_anything_is_launched():
    from fieldconv_amd import _lib
    lib = _lib.load()
    for N, C, dt, cplx, mode, B, thr, scale in ((4, 0, 0, 1, 0, 1, 0, 1.0), (-1, 4, 0, 1, 0, 1, 0, 1.0), (4, 4, 2, 1, 0, 1, 0, 1.0), (4, 4, 0, 2, 0, 1, 0, 1.0),
                                                (4, 4, 0, 1, 2, 1, 0, 1.0), (4, 4, 0, 1, 0, 0, 0, 1.0), (4, 4, 0, 1, 0, 1, (1 << 24) + 1, 1.0),
                                                (4, 4, 0, 1, 0, 1, 0, 0.0), (4, 4, 0, 1, 1, 2, 0, 1.0), (4, 4, 0, 1, 0, 1, 0, 2.0)):
        assert lib.fc_dropout(None, None, N, C, dt, cplx, mode, None, B, thr, scale, 1, 0, None, None) == -1
    assert lib.fc_dropout(None, None, 0, 4, 0, 1, 0, None, 1, 0, 1.0, 1, 0, None, None) == 0          # no rows: nothing to do
    assert lib.fc_philox_words(1, 2, 3, -1, None, None) == -1 and lib.fc_philox_words(1, 2, 3, 4, None, None) == -1
    assert lib.fc_philox_words(1, 2, 3, 0, None, None) == 0
    assert lib.fc_mesh_affine_draw(0, 1, 0, None, 0, 1.0, 1.0, 45.0, 45.0, 45.0, None, None, None) == -1
    assert lib.fc_mesh_affine_draw(2, 1, 0, None, 0, 1.0, 1.0, 45.0, 45.0, 45.0, None, None, None) == -1
    assert lib.fc_mesh_affine_apply(None, None, 1, 4, None, None, None, 4, None, None) == -1


def test_public_names():
    from fieldconv_amd import augment, dropout, functional, nn, transforms
    assert functional.tangent_dropout is dropout.tangent_dropout and functional.philox_words is dropout.philox_words
    assert functional.random_mesh_affine is augment.random_mesh_affine and functional.mesh_affine is augment.mesh_affine
    assert 'TangentDropout' in nn.__all__ and nn.__all__[-1] == 'MeshPool'
    assert 'RandomMeshAffine' in transforms.__all__ and transforms.RandomMeshAffine is not None


def test_module_state():
    from fieldconv_amd.nn import TangentDropout
    torch.manual_seed(7)
    a = TangentDropout()
    torch.manual_seed(7)
    b = TangentDropout(0.25, mode='channel')
    assert a.seed == b.seed and 0 <= a.seed < 2 ** 63          # torch.manual_seed governs the seed
    assert not a.state_dict() and not list(a.parameters())
    assert [n for n, _ in a.named_buffers()] == ['step'] and a.step.dtype == torch.int64 and tuple(a.step.shape) == (1,) and int(a.step) == 0
    assert a.p == 0.5 and a.mode == 'element' and TangentDropout(seed=5).seed == 5
    a.load_state_dict({})
    assert 'p=0.25' in repr(b) and "mode='channel'" in repr(b)
    x = torch.zeros(4, 3, dtype=torch.complex64)
    assert a.eval()(x) is x and int(a.step) == 0          # evaluation: x itself, no draw
    with pytest.raises(RuntimeError):
        a.train()(x)                                           # there is no CPU path
    for bad in (dict(p=1.0), dict(p=-0.1), dict(mode='row'), dict(seed=-1), dict(seed=2 ** 64), dict(seed=1.5)):
        with pytest.raises(ValueError):
            TangentDropout(**bad)


@pytest.mark.parametrize('change', ['p one', 'p negative', 'p nan', 'p bool', 'mode', 'x 1-d', 'x 3-d', 'no channels', 'x not a tensor',
                                    'seed negative', 'seed large', 'seed float', 'step negative', 'step dtype', 'step shape', 'ptr dtype',
                                    'ptr end', 'ptr descending', 'ptr 2-d', 'ptr short', 'training'])
def test_bad_arguments_raise_value_error(change):
    from fieldconv_amd.dropout import tangent_dropout
    x = torch.zeros(6, 4, dtype=torch.complex64)
    kw = dict(p=0.5, seed=SEED, step=0, ptr=torch.tensor([0, 2, 6]), mode='channel')
    if change == 'p one':
        kw['p'] = 1.0
    elif change == 'p negative':
        kw['p'] = -1e-3
    elif change == 'p nan':
        kw['p'] = float('nan')
    elif change == 'p bool':
        kw['p'] = False
    elif change == 'mode':
        kw['mode'] = 'row'
    elif change == 'x 1-d':
        x = x[:, 0]
    elif change == 'x 3-d':
        x = x[None]
    elif change == 'no channels':
        x = x[:, :0]
    elif change == 'x not a tensor':
        x = [[1j]]
    elif change == 'seed negative':
        kw['seed'] = -1
    elif change == 'seed large':
        kw['seed'] = 2 ** 64
    elif change == 'seed float':
        kw['seed'] = 1.5
    elif change == 'step negative':
        kw['step'] = -1
    elif change == 'step dtype':
        kw['step'] = torch.zeros(1, dtype=torch.int32)
    elif change == 'step shape':
        kw['step'] = torch.zeros(2, dtype=torch.int64)
    elif change == 'ptr dtype':
        kw['ptr'] = torch.tensor([0, 2, 6], dtype=torch.int32)
    elif change == 'ptr end':
        kw['ptr'] = torch.tensor([0, 2, 5])
    elif change == 'ptr descending':
        kw['ptr'] = torch.tensor([0, 4, 2, 6])
    elif change == 'ptr 2-d':
        kw['ptr'] = torch.tensor([[0, 6]])
    elif change == 'ptr short':
        kw['ptr'] = torch.tensor([6])
    elif change == 'training':
        kw['training'] = 1
    with pytest.raises(ValueError):
        tangent_dropout(x, **kw)


def test_other_dtypes_raise_type_error():
    from fieldconv_amd.dropout import tangent_dropout
    for dtype in (torch.float16, torch.bfloat16, torch.int32):
        with pytest.raises(TypeError):
            tangent_dropout(torch.zeros(6, 4, dtype=dtype), 0.5, SEED, 0)


def test_there_is_no_cpu_path():
    from fieldconv_amd.augment import mesh_affine
    from fieldconv_amd.dropout import tangent_dropout
    from fieldconv_amd.transforms import RandomMeshAffine
    for dtype in (torch.complex64, torch.complex128, torch.float32, torch.float64):
        x = torch.zeros(6, 4, dtype=dtype)
        with pytest.raises(RuntimeError):
            tangent_dropout(x, 0.5, SEED, 0)
        with pytest.raises(RuntimeError):
            tangent_dropout(x, 0.5, SEED, torch.zeros(1, dtype=torch.int64), torch.tensor([0, 2, 6]), 'channel')
        assert tangent_dropout(x, 0.5, SEED, 0, training=False) is x
    pos = torch.zeros(6, 3)
    with pytest.raises(RuntimeError):
        mesh_affine(pos, torch.tensor([0, 2, 6]), torch.zeros(2, 3, 3))

    class Mesh:
        pass
    mesh = Mesh()
    mesh.pos = pos
    with pytest.raises(RuntimeError):
        RandomMeshAffine(seed=1)(mesh)
    assert mesh.pos is pos


@pytest.mark.parametrize('change', ['pos dtype', 'pos shape', 'ptr end', 'M shape', 'M dtype', 't shape', 'index dtype', 'index 2-d'])
def test_bad_affine_arguments_raise_value_error(change):
    from fieldconv_amd.augment import mesh_affine
    pos, ptr, kw = torch.zeros(6, 3), torch.tensor([0, 2, 6]), dict(M=torch.zeros(2, 3, 3), t=torch.zeros(2, 3), index=torch.tensor([0, 5]))
    if change == 'pos dtype':
        pos = pos.double()
    elif change == 'pos shape':
        pos = torch.zeros(6, 2)
    elif change == 'ptr end':
        ptr = torch.tensor([0, 2, 7])
    elif change == 'M shape':
        kw['M'] = torch.zeros(3, 3, 3)
    elif change == 'M dtype':
        kw['M'] = torch.zeros(2, 3, 3, dtype=torch.float64)
    elif change == 't shape':
        kw['t'] = torch.zeros(2, 1)
    elif change == 'index dtype':
        kw['index'] = torch.tensor([0, 5], dtype=torch.int32)
    elif change == 'index 2-d':
        kw['index'] = torch.tensor([[0, 5]])
    with pytest.raises(ValueError):
        mesh_affine(pos, ptr, **kw)


def test_transform_arguments():
    from fieldconv_amd.augment import random_mesh_affine
    from fieldconv_amd.transforms import RandomMeshAffine
    torch.manual_seed(3)
    a = RandomMeshAffine()
    torch.manual_seed(3)
    b = RandomMeshAffine(scale=(0.85, 1.15), degrees=30, center=True)
    assert a.seed == b.seed and a.scale is None and b.degrees == (30.0, 30.0, 30.0) and a.degrees == (45.0, 45.0, 45.0) and a.step is None
    assert 'center=True' in repr(b) and RandomMeshAffine(seed=9).seed == 9
    for bad in (dict(scale=(1.2, 0.8)), dict(scale=(0.0, 1.0)), dict(scale=1.0), dict(degrees=(45, 45)), dict(degrees=-1), dict(degrees=(1, 2, 'x')),
                dict(center=1), dict(seed=-1)):
        with pytest.raises(ValueError):
            RandomMeshAffine(**bad)
    for bad in (dict(B=0, seed=1, step=0), dict(B=2, seed=-1, step=0), dict(B=2, seed=1, step=-1), dict(B=2, seed=1, step=0, scale=(2, 1)),
                dict(B=2, seed=1, step=torch.zeros(1))):
        with pytest.raises(ValueError):
            random_mesh_affine(**bad)
