"""The counter-based generator and TangentDropout on the device (fieldconv_amd.dropout, csrc/fc_philox.hpp, csrc/fc_dropout.hip,
nn.TangentDropout) against the numpy restatement tests/_philox_ref.py.

Everything here is an integer decision or one multiplication, so every comparison is BIT FOR BIT: the words, the masks, the values
and the gradients.  The shapes are the smallest that reach every route of the kernels: (0,5) launches nothing, (1,1) is a lone partial
Philox block, (7,5) is 35 entries and ends inside a block, (130,3) and (64,64) fill more than one workgroup's worth of blocks; a
misaligned view takes the scalar route of the element kernel, and one large case crosses the size from which the grid strides (2^26
entries) and byte offsets beyond 2^31."""
import functools

import numpy as np
import pytest
import torch

import _philox_ref as pref

pytestmark = pytest.mark.gpu

SEED = 2024
SHAPES = [(0, 5), (1, 1), (7, 5), (130, 3), (64, 64)]
PS = (0.0, 0.1, 0.5, 0.9)
DTYPES = {'complex64': (torch.complex64, np.complex64), 'complex128': (torch.complex128, np.complex128),
          'float32': (torch.float32, np.float32), 'float64': (torch.float64, np.float64)}
CHANNEL_CASES = [([0, 3, 3, 7], 5), ([0, 3, 3, 7], 64), ([0, 0, 1, 64, 129, 386], 3)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev=torch.device('cuda:0')):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.real.dtype == np.float64 else np.uint32)


def same(got, want):
    """bit for bit, signs of zeros included"""
    return got.dtype == want.dtype and got.shape == want.shape and np.array_equal(bits(got), bits(want))


@functools.lru_cache(maxsize=None)
def features(N, C, name, salt=0):
    """float32-representable entries without zeros, shared and never modified"""
    rng = np.random.default_rng(1000 * N + 10 * C + salt)
    re = rng.uniform(0.25, 2.0, (N, C)).astype(np.float32) * rng.choice([-1.0, 1.0], (N, C)).astype(np.float32)
    im = rng.uniform(0.25, 2.0, (N, C)).astype(np.float32) * rng.choice([-1.0, 1.0], (N, C)).astype(np.float32)
    npdt = DTYPES[name][1]
    return (re + 1j * im).astype(npdt) if np.issubdtype(npdt, np.complexfloating) else re.astype(npdt)


# ------------------------------------------------------------------ the raw words
@pytest.mark.parametrize('case', range(len(pref.KNOWN_ANSWERS)))
def test_device_words_equal_the_published_known_answers(dev, case):
    from fieldconv_amd.functional import philox_words
    counter, key, expected = pref.KNOWN_ANSWERS[case]
    got = philox_words(key[1] << 32 | key[0], counter[3] << 32 | counter[2], counter[1] << 32 | counter[0], 1, device=dev)
    assert got.dtype == torch.int64 and tuple(got.shape) == (1, 4) and got[0].tolist() == list(expected)


def test_device_words_carry_into_the_second_counter_word(dev):
    from fieldconv_amd.functional import philox_words
    for seed, hi, first, n in ((7, 9, 2 ** 32 - 2, 4), (2 ** 64 - 1, 2 ** 63 + 5, 2 ** 64 - 2, 4), (SEED, 3 | 2 << 32, 0, 600)):
        got = N_(philox_words(seed, hi, first, n, device=dev))
        assert np.array_equal(got, pref.words(seed, hi, first, n).astype(np.int64)), (seed, hi, first, n)
    assert tuple(philox_words(1, 2, 3, 0, device=dev).shape) == (0, 4)


# ------------------------------------------------------------------ values and gradients, element mode
@pytest.mark.parametrize('name', list(DTYPES))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_element_mode_equals_the_restatement_bit_for_bit(dev, shape, name):
    from fieldconv_amd.functional import tangent_dropout
    N, C = shape
    x, gy = features(N, C, name), features(N, C, name, 1)
    for p in PS:
        for step in (0, 3):
            keep = pref.element_keep(N, C, p, SEED, step)
            xd = T(x, dev).requires_grad_(True)
            y = tangent_dropout(xd, p, SEED, step)
            assert y.dtype == xd.dtype and y.data_ptr() != xd.data_ptr() or N == 0
            assert same(N_(y), pref.dropout(x, keep, p)), (p, step)
            (gx,) = torch.autograd.grad(y, xd, T(gy, dev))
            assert same(N_(gx), pref.dropout(gy, keep, p)), (p, step)          # gx = mask * scale * gy
            if p == 0.0:
                assert same(N_(y), x)                                        # a new tensor with x's bits
            elif N * C >= 35:
                assert 0 < int(keep.sum()) < N * C                           # (the case does drop and does keep)


def test_a_step_on_the_device_a_view_and_a_misaligned_tensor(dev):
    from fieldconv_amd.functional import tangent_dropout
    N, C, p = 130, 3, 0.5
    x = features(N, C, 'complex64')
    want = pref.dropout(x, pref.element_keep(N, C, p, SEED, 5), p)
    xd = T(x, dev)
    step = torch.tensor([5], dtype=torch.int64, device=dev)
    a, b = tangent_dropout(xd, p, SEED, step), tangent_dropout(xd, p, SEED, 5)
    assert same(N_(a), want) and same(N_(b), want)                           # the same (seed, step): the same bits
    assert not same(N_(tangent_dropout(xd, p, SEED, 6)), want) and not same(N_(tangent_dropout(xd, p, SEED + 1, 5)), want)
    step.add_(2 ** 32)                                                       # the low 32 bits of the step count
    assert same(N_(tangent_dropout(xd, p, SEED, step)), want)
    # a transposed view is made contiguous; a lazily conjugated one is resolved
    assert same(N_(tangent_dropout(T(np.ascontiguousarray(x.T), dev).t(), p, SEED, 5)), want)
    assert same(N_(tangent_dropout(T(np.conj(x), dev).conj(), p, SEED, 5)), want)
    # a contiguous tensor that starts 8 bytes into a 16-byte piece: the scalar route, the same bits
    for name in ('complex64', 'float32', 'float64'):
        flat = features(131, 3, name)
        big = T(flat, dev).reshape(-1)
        view = big[1:].reshape(-1, 1)
        assert view.is_contiguous() and view.data_ptr() % 16 != 0
        n = view.shape[0]
        assert same(N_(tangent_dropout(view, p, SEED, 1)), pref.dropout(flat.reshape(-1)[1:].reshape(-1, 1), pref.element_keep(n, 1, p, SEED, 1), p))
    assert tangent_dropout(xd, p, SEED, 5, training=False) is xd               # evaluation: x itself


def test_the_grid_stride_and_offsets_beyond_two_gib(dev):
    """2^21 + 1 rows of 65 complex128 entries: 1.36e8 entries (the grid strides from 2^26 on), 2.2e9 bytes each way.  Slices of the
    result are compared: the head, the entries around 2^26 and 2^27, and the tail, which ends inside a Philox block."""
    from fieldconv_amd.functional import tangent_dropout
    N, C, p = 2 ** 21 + 1, 65, 0.5
    total = N * C
    assert total > 2 ** 27 and total * 16 > 2 ** 31 and total % 4
    x = torch.full((N, C), 3.0 - 1.5j, dtype=torch.complex128, device=dev)
    y = tangent_dropout(x, p, SEED, 2).reshape(-1)
    for lo, hi in ((0, 1024), (2 ** 26 - 512, 2 ** 26 + 512), (2 ** 27 - 512, 2 ** 27 + 512), (total - 1023, total)):
        keep = pref.bits24(SEED, 2, pref.ELEMENT, np.arange(lo, hi, dtype=np.uint64)) >= np.uint64(pref.threshold(p))
        want = pref.dropout(np.full(hi - lo, 3.0 - 1.5j, dtype=np.complex128), keep, p)
        assert same(N_(y[lo:hi]), want), (lo, hi)
    kept = int((y.real != 0).sum())
    assert abs(kept - total / 2) <= 6 * np.sqrt(total / 4)


# ------------------------------------------------------------------ channel mode
@pytest.mark.parametrize('name', list(DTYPES))
@pytest.mark.parametrize('case', range(len(CHANNEL_CASES)))
def test_channel_mode_equals_the_restatement_bit_for_bit(dev, case, name):
    from fieldconv_amd.functional import tangent_dropout
    from fieldconv_amd.pooling import tag_ptr
    ptr, C = CHANNEL_CASES[case]
    N = ptr[-1]
    x, gy = features(N, C, name), features(N, C, name, 1)
    ptr_d = tag_ptr(torch.tensor(ptr, dtype=torch.int64).to(dev), ptr)          # as MeshBatch tags the tables it builds
    for p in PS:
        keep = pref.channel_keep(ptr, C, p, SEED, 1)
        for b in range(len(ptr) - 1):                                        # every row of a mesh shares its mesh's decision
            assert (keep[ptr[b]:ptr[b + 1]] == keep[ptr[b]:ptr[b] + 1]).all()
        xd = T(x, dev).requires_grad_(True)
        y = tangent_dropout(xd, p, SEED, 1, ptr_d, 'channel')
        assert same(N_(y), pref.dropout(x, keep, p)), p
        (gx,) = torch.autograd.grad(y, xd, T(gy, dev))
        assert same(N_(gx), pref.dropout(gy, keep, p)), p
    # a host ptr is moved; without ptr the tensor is one mesh; the element and the channel streams differ
    y = tangent_dropout(T(x, dev), 0.5, SEED, 1, torch.tensor(ptr), 'channel')
    assert same(N_(y), pref.dropout(x, pref.channel_keep(ptr, C, 0.5, SEED, 1), 0.5))
    one = pref.channel_keep([0, N], C, 0.5, SEED, 1)
    assert same(N_(tangent_dropout(T(x, dev), 0.5, SEED, 1, None, 'channel')), pref.dropout(x, one, 0.5))
    if C == 64:
        assert not np.array_equal(one, pref.element_keep(N, C, 0.5, SEED, 1))


# ------------------------------------------------------------------ the module
def test_module_draws_a_new_mask_every_training_call(dev):
    from fieldconv_amd.nn import TangentDropout
    m = TangentDropout(0.5, seed=SEED).to(dev)
    assert m.step.device.type == 'cuda' and not m.state_dict()
    x = features(64, 64, 'complex64')
    xd = T(x, dev)
    for step in range(3):
        assert int(m.step) == step
        assert same(N_(m(xd)), pref.dropout(x, pref.element_keep(64, 64, 0.5, SEED, step), 0.5))
    assert m.eval()(xd) is xd and int(m.step) == 3
    c = TangentDropout(0.1, mode='channel', seed=SEED + 1).to(dev)
    ptr = [0, 3, 3, 64]
    assert same(N_(c(xd, torch.tensor(ptr))), pref.dropout(x, pref.channel_keep(ptr, 64, 0.1, SEED + 1, 0), 0.1)) and int(c.step) == 1


def test_module_under_step_graph_draws_a_new_mask_on_every_replay(dev):
    from fieldconv_amd.nn import TangentDropout
    from fieldconv_amd.utils import StepGraph
    x, gy = features(130, 3, 'complex64'), features(130, 3, 'complex64', 1)
    m = TangentDropout(0.5, seed=SEED).to(dev)
    xd, gyd = T(x, dev).requires_grad_(True), T(gy, dev)

    def step():
        y = m(xd)
        return (y.detach(),) + torch.autograd.grad(y, xd, gyd)
    graphed = StepGraph(step)
    masks = []
    for _ in range(2):
        s = int(m.step)                                                      # the step this replay draws with
        y, gx = (N_(t) for t in graphed.replay())
        keep = pref.element_keep(130, 3, 0.5, SEED, s)
        assert same(y, pref.dropout(x, keep, 0.5)) and same(gx, pref.dropout(gy, keep, 0.5)), s
        assert int(m.step) == s + 1
        masks.append(keep)
    assert not np.array_equal(masks[0], masks[1])
