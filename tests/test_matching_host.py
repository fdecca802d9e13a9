"""Host-side tests of descriptor matching (fieldconv_amd.matching, utils.hard_null_pairs): the numpy restatement the GPU tests
compare with (tests/_matching_ref.py) against a brute-force double loop, the public surface, and the argument checks that need
no device."""
import numpy as np
import pytest
import torch

import _matching_ref as mref


def _brute(xS, xT, k, seg=None, exclude=None):
    """Every pair by two Python loops, the distance channel by channel in the arrays' dtype, candidates sorted as (d2, b) tuples."""
    dt = xT.dtype.type
    idx = np.full((xT.shape[0], k), -1, dtype=np.int64)
    d2 = np.full((xT.shape[0], k), np.inf, dtype=xT.dtype)
    for a in range(xT.shape[0]):
        lo, hi = (0, xS.shape[0]) if seg is None else seg(a)
        cand = []
        for b in range(lo, hi):
            acc = dt(0)
            for c in range(xT.shape[1]):
                t = dt(xT[a, c] - xS[b, c])
                acc = dt(acc + dt(t * t))
            if not np.isnan(acc) and not (exclude is not None and exclude[a] == b):
                cand.append((acc, b))
        for j, (d, b) in enumerate(sorted(cand)[:k]):
            idx[a, j], d2[a, j] = b, d
    return idx, d2


def _same(got, want):
    bits = np.uint32 if want[1].dtype == np.float32 else np.uint64
    return np.array_equal(got[0], want[0]) and got[1].dtype == want[1].dtype and np.array_equal(got[1].view(bits), want[1].view(bits))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_restatement_equals_brute_force(dtype):
    rng = np.random.default_rng(0)
    N, C = 7, 5
    cases = [(rng.random((N, C)).astype(dtype), rng.random((N, C)).astype(dtype)),
             (rng.integers(-2, 3, (N, C)).astype(dtype), rng.integers(-2, 3, (N, C)).astype(dtype))]          # exact ties
    ties = cases[1][0].copy()
    ties[4] = ties[1]                                                                                          # a duplicated row
    cases.append((ties, cases[1][1]))
    nan = cases[0][0].copy()
    nan[2] = np.nan
    cases.append((nan, cases[0][1]))
    for xS, xT in cases:
        for k in (1, 3, 8):
            assert _same(mref.topk(xS, xT, k), _brute(xS, xT, k))
            exclude = np.array([-1, 0, 6, 3, -1, 2, 2])
            assert _same(mref.topk(xS, xT, k, exclude=exclude), _brute(xS, xT, k, exclude=exclude))
            ptr_T, ptr_S = [0, 3, 3, 7], [0, 2, 6, 7]

            def seg(a):
                m = 0 if a < 3 else 2
                return ptr_S[m], ptr_S[m + 1]
            assert _same(mref.topk(xS, xT, k, ptr_S, ptr_T), _brute(xS, xT, k, seg=seg))
            rows = np.array([5, 0, 3])
            full = mref.topk(xS, xT, k, ptr_S, ptr_T, exclude)
            assert _same(mref.topk(xS, xT, k, ptr_S, ptr_T, exclude, rows=rows), (full[0][rows], full[1][rows]))
    # the lower row wins an exact tie; a NaN row of xS is never returned, a NaN row of xT matches nothing
    idx, _ = mref.topk(ties, ties, 2)
    assert list(idx[1]) == [1, 4] and list(idx[4]) == [1, 4]
    idx, d2 = mref.topk(nan, nan, 8)
    assert not (idx == 2).any() and (idx[2] == -1).all() and np.isinf(d2[2]).all() and (idx[0, :6] >= 0).all() and idx[0, 6] == -1


def test_restated_mutual_accuracy_hard():
    xS = np.array([[0.0], [1.0], [5.0], [5.25]], dtype=np.float32)
    xT = np.array([[0.9], [0.1], [5.1], [9.0]], dtype=np.float32)
    assert mref.mutual(xS, xT).tolist() == [[0, 1], [1, 0], [2, 2]]          # xT[3]'s nearest is xS[3], whose nearest is xT[2]
    idx, _ = mref.topk(xS, xT, 2)
    pos = np.array([[0, 1], [1, 1], [2, 3], [2, 3]])
    assert mref.accuracy(idx, pos).tolist() == [1 / 3, 1.0]
    assert mref.hard_negatives(xS, xT, np.array([[2, 2], [0, 1]]), 2).tolist() == [[0, 0], [0, 2], [2, 3], [2, 1]]


def test_names_exported():
    from fieldconv_amd import functional, matching, utils
    for name in ('match_descriptors', 'mutual_matches', 'match_accuracy'):
        assert getattr(functional, name) is getattr(matching, name)
    assert callable(utils.hard_null_pairs) and 'hard_null_pairs' in utils.__all__


def test_match_accuracy_is_plain_torch():
    from fieldconv_amd.functional import match_accuracy
    idx = torch.tensor([[1, 0], [0, 1], [2, 3], [3, 2]])
    pos = torch.tensor([[0, 1], [1, 1], [2, 3], [2, 3]])
    acc = match_accuracy(idx, pos)
    assert acc.dtype == torch.float64 and acc.tolist() == [1 / 3, 1.0]
    assert np.array_equal(acc.numpy(), mref.accuracy(idx.numpy(), pos.numpy()))
    with pytest.raises(ValueError):
        match_accuracy(idx, pos[:0])
    with pytest.raises(ValueError):
        match_accuracy(idx.to(torch.int32), pos)


def test_bad_arguments_raise():
    from fieldconv_amd.functional import match_descriptors, mutual_matches
    from fieldconv_amd.utils import hard_null_pairs
    xS, xT = torch.rand(10, 16), torch.rand(12, 16)
    with pytest.raises(RuntimeError, match='no CPU path'):
        match_descriptors(xS, xT)
    with pytest.raises(RuntimeError, match='no CPU path'):
        mutual_matches(xS, xT)
    for k in (0, 9, 1.5, True):
        with pytest.raises(ValueError, match='k must be'):
            match_descriptors(xS, xT, k=k)
    for parts in (-1, 1025):
        with pytest.raises(ValueError, match='parts must be'):
            match_descriptors(xS, xT, parts=parts)
    with pytest.raises(ValueError, match='channel count'):
        match_descriptors(xS, xT[:, :15])
    with pytest.raises(ValueError, match='channel count'):
        match_descriptors(xS, xT.double())
    with pytest.raises(ValueError):
        match_descriptors(xS, xT[0])
    ptr = torch.tensor([0, 12])
    for kw in (dict(ptr_T=ptr), dict(ptr_S=torch.tensor([0, 10]))):
        with pytest.raises(ValueError, match='go together'):
            match_descriptors(xS, xT, **kw)
    for exclude in (torch.zeros(10, dtype=torch.int64), torch.zeros(12, dtype=torch.int32), torch.zeros((12, 1), dtype=torch.int64), [0] * 12):
        with pytest.raises(ValueError, match='exclude must be'):
            match_descriptors(xS, xT, exclude=exclude)
    # hard negatives: one positive per row; a well-formed list then reaches the device check
    with pytest.raises(ValueError, match='more than one distinct positive'):
        hard_null_pairs(xS, xT, torch.tensor([[0, 1], [3, 2], [0, 4]]))
    with pytest.raises(IndexError):
        hard_null_pairs(xS, xT, torch.tensor([[12, 0]]))
    with pytest.raises(RuntimeError, match='no CPU path'):
        hard_null_pairs(xS, xT, torch.tensor([[0, 1], [3, 2], [0, 1]]))          # a repeated pair is one positive
