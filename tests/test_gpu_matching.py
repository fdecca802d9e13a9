"""Descriptor matching on the device (fieldconv_amd.matching, csrc/fc_match.hip; utils.hard_null_pairs) against the numpy
restatement tests/_matching_ref.py.  Every comparison with the restatement is exact: the same idx and the same bits of d2 -- the
kernel's distance is the losses' (one definition) and the order (d2, b) is total, so there is nothing to tolerate.  Shapes sit
where the 64 x 64 x 16-channel tile can go wrong: one row, sizes just under / at / over a tile and a channel chunk, several tiles."""
import ctypes

import numpy as np
import pytest
import torch

import _matching_ref as mref

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 1), (3, 2, 16), (64, 64, 16), (65, 63, 17), (130, 129, 33), (200, 257, 5)]          # (N_T, N_S, C)
KS = (1, 3, 8)
DTYPES = [(np.float32, torch.float32), (np.float64, torch.float64)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(got, want):
    """(idx, d2) device tensors against the restatement's arrays: equal indices, equal bits"""
    gi, gd = N_(got[0]), N_(got[1])
    assert gi.dtype == np.int64 and gd.dtype == want[1].dtype and gi.shape == want[0].shape and gd.shape == want[1].shape
    return np.array_equal(gi, want[0]) and np.array_equal(bits(gd), bits(want[1]))


def features(n_T, n_S, C, seed, ndt):
    rng = np.random.default_rng(seed)
    return (0.9 * rng.random((n_S, C))).astype(ndt), (0.9 * rng.random((n_T, C))).astype(ndt)


# ------------------------------------------------------------------ the contract, shape by shape
@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('n_T,n_S,C', SHAPES)
def test_matches_equal_the_restatement(dev, n_T, n_S, C, ndt, dt):
    from fieldconv_amd.functional import match_descriptors
    xS, xT = features(n_T, n_S, C, seed=n_T + C, ndt=ndt)
    for k in KS:                                                   # k > N_S at the two smallest shapes: the tail is -1 / +inf
        idx, d2 = match_descriptors(T(xS, dev), T(xT, dev), k=k)
        assert idx.dtype == torch.int64 and d2.dtype == dt and tuple(idx.shape) == tuple(d2.shape) == (n_T, k)
        assert same((idx, d2), mref.topk(xS, xT, k)), (k,)
        if k > n_S:
            assert bool((idx[:, n_S:] == -1).all()) and bool(torch.isinf(d2[:, n_S:]).all()) and bool((idx[:, :n_S] >= 0).all())


@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_exact_ties_go_to_the_lower_row(dev, ndt, dt):
    """Integer features in [-2, 2] with 5 channels: most rows of xT have several rows of xS at exactly the smallest distance.
    Duplicated rows of xS on top (also across a tile boundary and in different lanes' columns)."""
    from fieldconv_amd.functional import match_descriptors
    n_T, n_S, C = 200, 257, 5
    rng = np.random.default_rng(7)
    xS, xT = rng.integers(-2, 3, (n_S, C)).astype(ndt), rng.integers(-2, 3, (n_T, C)).astype(ndt)
    xS[[70, 131, 256]] = xS[3]
    xS[200] = xS[199]
    xT[:8] = xS[[3, 70, 131, 256, 199, 200, 0, 1]]
    D = mref.ref.dense_sqdist(xT, xS)
    assert ((D == D.min(1, keepdims=True)).sum(1) >= 2).mean() > 0.5          # ties for FIRST place in most rows
    for k in KS:
        got = match_descriptors(T(xS, dev), T(xT, dev), k=k)
        assert same(got, mref.topk(xS, xT, k)), (k,)
    idx = N_(match_descriptors(T(xS, dev), T(xT, dev), k=8)[0])
    assert (idx[:4, :4] == [3, 70, 131, 256]).all() and (idx[4:6, :2] == [199, 200]).all()
    d = np.take_along_axis(D, idx, 1)
    assert ((np.diff(d, axis=1) > 0) | ((np.diff(d, axis=1) == 0) & (np.diff(idx, axis=1) > 0))).all()          # (d2, b) strictly ascending


@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_nan_is_never_a_match(dev, ndt, dt):
    from fieldconv_amd.functional import match_descriptors
    n_T, n_S, C = 130, 129, 17
    xS, xT = features(n_T, n_S, C, seed=3, ndt=ndt)
    xS[[0, 64, 128]] = np.nan          # whole rows
    xS[5, 16] = np.nan                 # one channel, in the second chunk
    xT[[1, 77]] = np.nan
    for k in KS:
        idx, d2 = match_descriptors(T(xS, dev), T(xT, dev), k=k)
        assert same((idx, d2), mref.topk(xS, xT, k))
        assert not bool(torch.isin(idx, torch.tensor([0, 5, 64, 128], device=dev)).any()) and not bool(torch.isnan(d2).any())
        assert bool((idx[[1, 77]] == -1).all()) and bool(torch.isinf(d2[[1, 77]]).all()) and bool((idx[0] >= 0).all())
    # every row of xS NaN: nothing matches anywhere
    idx, d2 = match_descriptors(T(np.full_like(xS, np.nan), dev), T(xT, dev), k=3, parts=2)
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all())


@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_result_does_not_depend_on_parts(dev, ndt, dt):
    from fieldconv_amd.functional import match_descriptors
    n_T, n_S, C = 130, 1000, 16
    rng = np.random.default_rng(11)
    xS, xT = features(n_T, n_S, C, seed=11, ndt=ndt)
    xS[rng.integers(0, n_S, 300)] = xS[rng.integers(0, n_S, 300)]          # duplicated rows: exact ties across the parts' ranges
    for k in (1, 8):
        want = mref.topk(xS, xT, k)
        auto = match_descriptors(T(xS, dev), T(xT, dev), k=k, parts=0)
        assert same(auto, want)
        for parts in (1, 2, 5, 16, 16):          # (16 twice: two runs give the same bits)
            got = match_descriptors(T(xS, dev), T(xT, dev), k=k, parts=parts)
            assert torch.equal(got[0], auto[0]) and np.array_equal(bits(N_(got[1])), bits(N_(auto[1]))), (k, parts)
    # more parts than tiles of xS: the surplus parts are empty
    xS, xT = features(70, 100, 3, seed=12, ndt=ndt)
    assert same(match_descriptors(T(xS, dev), T(xT, dev), k=3, parts=7), mref.topk(xS, xT, 3))


@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('parts', [1, 3])
@pytest.mark.parametrize('k', [1, 2, 3, 4, 5, 8])
def test_every_rung_of_the_list_ladder(dev, k, parts, ndt, dt):
    """Every list length the kernels are compiled for (1, 2, 4, 8), filled (k = K) and not (k = 3, 5), from one part and merged
    from three.  65 rows of xT: a second tile; 130 rows of xS: three tiles, so that each of three parts has one."""
    from fieldconv_amd.functional import match_descriptors
    xS, xT = features(65, 130, 5, seed=21, ndt=ndt)
    xS[[64, 129]] = xS[2]          # exact ties across the parts' ranges
    assert same(match_descriptors(T(xS, dev), T(xT, dev), k=k, parts=parts), mref.topk(xS, xT, k))


# ------------------------------------------------------------------ segments (the meshes of two mini-batches)
@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_segments(dev, ndt, dt):
    """B = 4, ranges that are no multiples of 64: an empty xT segment, an empty xS segment (its xT rows match nothing) and an xS
    segment shorter than k.  Equal to the restatement, and to single calls on the slices with idx offset."""
    from fieldconv_amd.functional import match_descriptors
    from fieldconv_amd.pooling import tag_ptr
    ptr_T, ptr_S = [0, 70, 70, 200, 333], [0, 130, 150, 150, 155]
    xS, xT = features(ptr_T[-1], ptr_S[-1], 17, seed=5, ndt=ndt)
    dS, dT = T(xS, dev), T(xT, dev)
    pT, pS = tag_ptr(T(np.array(ptr_T), dev), ptr_T), torch.tensor(ptr_S)          # a tagged device table, a host table
    for k, parts in ((1, 0), (3, 2), (8, 1), (8, 3)):
        got = match_descriptors(dS, dT, k=k, ptr_S=pS, ptr_T=pT, parts=parts)
        assert same(got, mref.topk(xS, xT, k, ptr_S, ptr_T)), (k, parts)
        idx, d2 = got
        assert bool((idx[70:200] == -1).all()) and bool(torch.isinf(d2[70:200]).all())          # the empty xS segment
        assert bool((idx[200:, :min(k, 5)] >= 150).all()) and bool((idx[200:, 5:] == -1).all())          # five rows to choose from
        for m in (0, 3):
            t0, t1, s0, s1 = ptr_T[m], ptr_T[m + 1], ptr_S[m], ptr_S[m + 1]
            si, sd = match_descriptors(dS[s0:s1], dT[t0:t1], k=k, parts=parts)
            assert torch.equal(torch.where(si >= 0, si + s0, si), idx[t0:t1]) and np.array_equal(bits(N_(sd)), bits(N_(d2[t0:t1])))
    with pytest.raises(ValueError):
        match_descriptors(dS, dT, ptr_S=pS, ptr_T=torch.tensor([0, 70, 333]))          # another number of meshes
    with pytest.raises(ValueError):
        match_descriptors(dS, dT, ptr_S=pS, ptr_T=torch.tensor([0, 70, 70, 200, 300]))          # does not end at N_T


# ------------------------------------------------------------------ exclude
@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_exclude(dev, ndt, dt):
    from fieldconv_amd.functional import match_descriptors
    n_T, n_S, C = 130, 129, 16
    xS, xT = features(n_T, n_S, C, seed=9, ndt=ndt)
    rng = np.random.default_rng(9)
    nearest = mref.topk(xS, xT, 1)[0][:, 0]
    exclude = np.where(rng.random(n_T) < 0.7, nearest, rng.integers(0, n_S, n_T))          # mostly the row that would have won
    exclude[::10] = -1
    for k, parts in ((1, 0), (3, 1), (8, 4)):
        idx, d2 = match_descriptors(T(xS, dev), T(xT, dev), k=k, exclude=T(exclude, dev), parts=parts)
        assert same((idx, d2), mref.topk(xS, xT, k, exclude=exclude))
        assert not bool((idx == T(exclude, dev)[:, None]).any())
        plain = match_descriptors(T(xS, dev), T(xT, dev), k=k, parts=parts)
        none = match_descriptors(T(xS, dev), T(xT, dev), k=k, exclude=torch.full((n_T,), -1, device=dev), parts=parts)
        assert torch.equal(plain[0], none[0]) and torch.equal(plain[1], none[1])
    # one row of xS and that row excluded: nothing is left
    idx, d2 = match_descriptors(T(xS[:1], dev), T(xT, dev), k=3, exclude=torch.zeros(n_T, dtype=torch.int64, device=dev))
    assert bool((idx == -1).all()) and bool(torch.isinf(d2).all())
    with pytest.raises(RuntimeError):
        match_descriptors(T(xS, dev), T(xT, dev), exclude=torch.zeros(n_T, dtype=torch.int64))          # on the host


# ------------------------------------------------------------------ consistency with the losses
@pytest.mark.parametrize('ndt,dt', DTYPES, ids=['f32', 'f64'])
def test_distance_is_pair_sqdist_bit_for_bit(dev, ndt, dt):
    """Also the tensor contract: non-contiguous views and tensors that require grad are taken; the outputs carry no graph."""
    from fieldconv_amd.functional import match_descriptors
    from fieldconv_amd.losses import pair_sqdist
    n_T, n_S, C = 200, 257, 33
    xS, xT = features(n_T, n_S, 2 * C, seed=13, ndt=ndt)
    vS, vT = T(xS, dev)[:, ::2].requires_grad_(True), T(xT.T.copy(), dev).T[:, ::2]
    assert not vS.is_contiguous() and not vT.is_contiguous()
    idx, d2 = match_descriptors(vS, vT, k=3)
    assert not idx.requires_grad and not d2.requires_grad
    assert same((idx, d2), mref.topk(xS[:, ::2], xT[:, ::2], 3))
    for j in range(3):
        pairs = torch.stack((torch.arange(n_T, device=dev), idx[:, j]), 1)
        assert torch.equal(pair_sqdist(vS, vT, pairs), d2[:, j])


# ------------------------------------------------------------------ mutual matches, accuracy, hard negatives on a planted problem
@pytest.fixture(scope='module')
def planted():
    """xT is a permutation of xS plus small noise, 10 % of its rows replaced by unrelated ones"""
    rng = np.random.default_rng(21)
    n, C = 300, 16
    xS = rng.random((n, C)).astype(np.float32)
    perm = rng.permutation(n)
    xT = (xS[perm] + 0.2 * rng.standard_normal((n, C))).astype(np.float32)          # (some planted rows lose their first place)
    replaced = rng.permutation(n)[:n // 10]
    xT[replaced] = rng.random((replaced.size, C)).astype(np.float32)
    kept = np.setdiff1d(np.arange(n), replaced)
    pos = np.stack((kept, perm[kept]), 1)[rng.permutation(kept.size)]          # the positives, in no particular order
    return xS, xT, pos


def test_mutual_matches_and_accuracy(dev, planted):
    from fieldconv_amd.functional import match_accuracy, match_descriptors, mutual_matches
    xS, xT, pos = planted
    got = mutual_matches(T(xS, dev), T(xT, dev))
    want = mref.mutual(xS, xT)
    assert got.dtype == torch.int64 and np.array_equal(N_(got), want)
    found = {(a, b) for a, b in want.tolist()} & {(a, b) for a, b in pos.tolist()}
    assert len(found) > 0.8 * pos.shape[0] and want.shape[0] < xT.shape[0]          # the planted matches, not the replaced rows
    idx, _ = match_descriptors(T(xS, dev), T(xT, dev), k=8)
    acc = match_accuracy(idx, T(pos, dev))
    assert acc.dtype == torch.float64 and tuple(acc.shape) == (8,)
    assert np.array_equal(N_(acc), mref.accuracy(N_(idx), pos))
    assert 0.9 < acc[0] < acc[-1] < 1 and bool((acc[1:] >= acc[:-1]).all())
    # with tables: two meshes of 150 rows match inside themselves
    ptr = torch.tensor([0, 150, 300])
    got = mutual_matches(T(xS, dev), T(xT, dev), ptr_S=ptr, ptr_T=ptr)
    assert np.array_equal(N_(got), mref.mutual(xS, xT, [0, 150, 300], [0, 150, 300]))
    assert bool(((got[:, 0] < 150) == (got[:, 1] < 150)).all())


def test_hard_null_pairs(dev, planted):
    from fieldconv_amd.losses import twin_loss
    from fieldconv_amd.utils import hard_null_pairs
    xS, xT, pos = planted
    dpos = T(np.concatenate((pos, pos[:20])), dev)          # a repeated pair is still one positive
    for per_row in (1, 3):
        neg = hard_null_pairs(T(xS, dev), T(xT, dev), dpos, per_row=per_row)
        assert neg.dtype == torch.int64 and tuple(neg.shape) == (pos.shape[0] * per_row, 2)
        assert np.array_equal(N_(neg), mref.hard_negatives(xS, xT, pos, per_row))
        assert bool((neg >= 0).all()) and int(neg[:, 0].max()) < xT.shape[0] and int(neg[:, 1].max()) < xS.shape[0]
        lin = N_(neg[:, 0] * xS.shape[0] + neg[:, 1])
        assert not np.isin(lin, pos[:, 0] * xS.shape[0] + pos[:, 1]).any() and np.unique(lin).size == lin.size
        assert bool((neg[1:, 0] >= neg[:-1, 0]).all())
    a, b = T(xS, dev).requires_grad_(True), T(xT, dev).requires_grad_(True)
    loss = twin_loss(a, b, dpos, neg, 0.2 * torch.rand(neg.shape[0], device=dev), 5)
    gS, gT = torch.autograd.grad(loss, [a, b])
    assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(gS).all()) and bool(torch.isfinite(gT).all()) and bool(gS.abs().max() > 0)
    # a feature matrix with two rows and one of them the positive: one slot comes back, the other is dropped
    few = hard_null_pairs(T(xS[:2], dev), T(xT, dev), T(np.array([[4, 1], [9, 0]]), dev), per_row=2)
    assert N_(few).tolist() == [[4, 0], [9, 1]]
    with pytest.raises(ValueError):
        hard_null_pairs(T(xS, dev), T(xT, dev), T(np.array([[4, 1], [4, 2]]), dev))


# ------------------------------------------------------------------ guard bands and the workspace contract
GUARD = 4096
PATTERN = 0xA5


def _guarded(nbytes, dev):
    buf = torch.full((GUARD + nbytes + GUARD,), PATTERN, dtype=torch.uint8, device=dev)
    return buf, buf[GUARD:GUARD + nbytes]


def _intact(buf, nbytes):
    return bool((buf[:GUARD] == PATTERN).all()) and bool((buf[GUARD + nbytes:] == PATTERN).all())


@pytest.mark.parametrize('n_T,n_S,C,k,parts', [(130, 300, 17, 3, 4), (65, 63, 5, 8, 16), (1, 1, 1, 1, 2), (200, 257, 16, 5, 0), (130, 129, 33, 8, 1)])
def test_no_write_outside_any_buffer(dev, n_T, n_S, C, k, parts):
    """idx, d2 and the workspace carved out of larger allocations filled with a byte pattern: the margins are intact after the call,
    the call succeeds with exactly fc_match_workspace_bytes and returns FC_ERR_WORKSPACE with one byte less."""
    from fieldconv_amd import _lib
    lib = _lib.load()
    vp = ctypes.c_void_p
    for ndt, code in ((np.float32, 0), (np.float64, 1)):
        xS, xT = features(n_T, n_S, C, seed=n_T + k, ndt=ndt)
        dS, dT = T(xS, dev), T(xT, dev)
        nbytes = lib.fc_match_workspace_bytes(n_T, k, parts)
        # O(N_T k parts): 12 bytes per entry and two roundings to 256 bytes; parts = 0 may choose up to 1024 / tiles of xT
        most = parts if parts else max(1, 1024 // ((n_T + 63) // 64))
        assert nbytes <= 12 * n_T * k * most + 512 and (nbytes > 0) == (most > 1)
        itemsize = np.dtype(ndt).itemsize
        bufs = [_guarded(n, dev) for n in (8 * n_T * k, itemsize * n_T * k, nbytes)]
        (_, idx), (_, d2), (_, ws) = bufs
        stream = vp(torch.cuda.current_stream().cuda_stream)

        def call(ws_bytes):
            return lib.fc_match_topk(vp(dS.data_ptr()), n_S, vp(dT.data_ptr()), n_T, C, code, None, None, 0, None, k, parts, vp(idx.data_ptr()),
                                     vp(d2.data_ptr()), vp(ws.data_ptr()) if nbytes else None, ws_bytes, stream)
        assert call(nbytes) == 0
        torch.cuda.synchronize()
        assert all(_intact(buf, view.numel()) for buf, view in bufs)
        got = idx.view(torch.int64).view(n_T, k), d2.view(torch.float32 if code == 0 else torch.float64).view(n_T, k)
        assert same(got, mref.topk(xS, xT, k))
        if nbytes:
            assert call(nbytes - 1) == -4          # FC_ERR_WORKSPACE
        assert lib.fc_match_topk(vp(dS.data_ptr()), n_S, vp(dT.data_ptr()), n_T, C, code, None, None, 0, None, 9, parts, vp(idx.data_ptr()),
                                 vp(d2.data_ptr()), None, 0, stream) == -1          # FC_ERR_BAD_ARGUMENT: k


def test_memory_stays_linear_at_20000_rows(dev):
    """N_T = N_S = 20 000, C = 16, k = 1: the call's peak allocation grows by less than 64 MB (the distance matrix alone would be
    1.6 GB); 256 random rows against the restatement."""
    from fieldconv_amd.functional import match_descriptors
    n, C = 20000, 16
    xS, xT = features(n, n, C, seed=1, ndt=np.float32)
    dS, dT = T(xS, dev), T(xT, dev)
    match_descriptors(dS[:64], dT[:64])          # (the library is loaded)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    idx, d2 = match_descriptors(dS, dT, k=1)
    torch.cuda.synchronize()
    grown = torch.cuda.max_memory_allocated() - before
    print('peak allocation growth', grown, 'bytes')
    assert grown < 64 * 2 ** 20
    rows = np.random.default_rng(2).permutation(n)[:256]
    want = mref.topk(xS, xT, 1, rows=rows)
    assert same((idx[T(rows, dev)], d2[T(rows, dev)]), want)


# ------------------------------------------------------------------ StepGraph
def test_match_replays_in_a_step_graph(dev):
    from fieldconv_amd.functional import match_descriptors
    from fieldconv_amd.utils import StepGraph
    n_T, n_S, C = 200, 300, 16
    xS, xT = features(n_T, n_S, C, seed=31, ndt=np.float32)
    dS, dT = T(xS, dev), T(xT, dev)
    exclude = torch.full((n_T,), -1, device=dev)
    graphed = StepGraph(lambda: match_descriptors(dS, dT, k=3, exclude=exclude))
    assert same(graphed.replay(), mref.topk(xS, xT, 3))
    for seed in (32, 33):
        xS, xT = features(n_T, n_S, C, seed=seed, ndt=np.float32)
        dS.copy_(T(xS, dev))
        dT.copy_(T(xT, dev))
        ex = np.full(n_T, -1)
        ex[:50] = mref.topk(xS, xT, 1)[0][:50, 0]
        exclude.copy_(T(ex, dev))
        assert same(graphed.replay(), mref.topk(xS, xT, 3, exclude=ex))
