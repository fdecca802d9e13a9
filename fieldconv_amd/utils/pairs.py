"""Pair lists for the feature-matching loop (TwinLoss / TwinEval) without the N_T x N_S complement ever existing.

A pair is a row [a, b] = [row of xT, row of xS]; its linear index is a * n_S + b.  The null (negative) pairs are the
complement of the DISTINCT positive pairs in [0, n_T) x [0, n_S), in ascending linear index.  Index arithmetic in plain
torch on whatever device the positives are on (CPU tensors are fine here: these are indices, not features); memory is
O(P log P + n), never O(n_T * n_S).

The reference's notebook builds the complement with np.setdiff1d over all n^2 indices, and indexes rows of its positive
list where it means columns, so it removes 2 indices rather than P; this module removes the positives."""
import torch


def _sorted_positive_index(pos_pairs, n_T, n_S, what):
    if isinstance(n_T, bool) or isinstance(n_S, bool) or int(n_T) != n_T or int(n_S) != n_S or n_T < 1 or n_S < 1:
        raise ValueError(f'{what}: n_T and n_S must be integers >= 1, got {n_T!r}, {n_S!r}')
    if int(n_T) * int(n_S) >= 2 ** 62:
        raise ValueError(f'{what}: n_T * n_S must stay below 2^62')
    if not torch.is_tensor(pos_pairs) or pos_pairs.dim() != 2 or pos_pairs.shape[1] != 2 or pos_pairs.dtype != torch.int64:
        raise ValueError(f'{what}: pos_pairs must be a (P,2) int64 tensor of [row of xT, row of xS]')
    if pos_pairs.shape[0]:
        lo, hi = pos_pairs.amin(0), pos_pairs.amax(0)
        if bool((lo[0] < 0) | (lo[1] < 0) | (hi[0] >= n_T) | (hi[1] >= n_S)):
            raise IndexError(f'{what}: positive pair outside [0, {n_T}) x [0, {n_S})')
    return torch.unique(pos_pairs[:, 0] * int(n_S) + pos_pairs[:, 1])          # sorted ascending, duplicates removed


def null_pair_count(pos_pairs, n_T, n_S):
    """Number of pairs of [0, n_T) x [0, n_S) that are not in pos_pairs (duplicates in pos_pairs count once)."""
    return int(n_T) * int(n_S) - int(_sorted_positive_index(pos_pairs, n_T, n_S, 'null_pair_count').numel())


def _from_rank(sorted_pos, n_S, rank):
    # the r-th non-positive index skips every positive at or below it: positive j (0-based, ascending) is skipped by the
    # ranks r >= sorted_pos[j] - j
    lin = rank + torch.searchsorted(sorted_pos - torch.arange(sorted_pos.numel(), device=sorted_pos.device), rank, right=True)
    return torch.stack((torch.div(lin, int(n_S), rounding_mode='floor'), lin % int(n_S)), 1)


def null_pairs_from_rank(pos_pairs, n_T, n_S, rank):
    """(R,2) int64: for each entry r of `rank` (int64, 0 <= r < null_pair_count), the r-th null pair in ascending linear
    index."""
    sorted_pos = _sorted_positive_index(pos_pairs, n_T, n_S, 'null_pairs_from_rank')
    if not torch.is_tensor(rank) or rank.dim() != 1 or rank.dtype != torch.int64 or rank.device != pos_pairs.device:
        raise ValueError('null_pairs_from_rank: rank must be a 1-D int64 tensor on the device of pos_pairs')
    count = int(n_T) * int(n_S) - int(sorted_pos.numel())
    if rank.numel() and (int(rank.min()) < 0 or int(rank.max()) >= count):
        raise IndexError(f'null_pairs_from_rank: rank outside [0, {count})')
    return _from_rank(sorted_pos, n_S, rank)


def _distinct_ranks(count, n, device, generator):
    """n distinct integers of [0, count), uniform over the n-subsets, in random order, in O(n) memory: draw with
    replacement, keep first occurrences, top up until n are there (a permutation when n is a large part of count)."""
    if 2 * n >= count:
        return torch.randperm(count, device=device, generator=generator)[:n]
    got = torch.empty(0, dtype=torch.int64, device=device)
    while got.numel() < n:
        draw = torch.randint(count, (n - got.numel() + 16,), device=device, generator=generator, dtype=torch.int64)
        both = torch.cat((got, draw))
        # first occurrences, in drawing order
        srt, order = torch.sort(both, stable=True)
        first = torch.ones_like(srt, dtype=torch.bool)
        first[1:] = srt[1:] != srt[:-1]
        got = both[torch.sort(order[first])[0]][:n]
    return got


def sample_null_pairs(pos_pairs, n_T, n_S, n, generator=None):
    """(n,2) int64: n distinct null pairs drawn uniformly (every n-subset of the complement equally likely), on the device
    of pos_pairs.  `generator` must live on that device; None is torch's global generator there."""
    sorted_pos = _sorted_positive_index(pos_pairs, n_T, n_S, 'sample_null_pairs')
    count = int(n_T) * int(n_S) - int(sorted_pos.numel())
    if isinstance(n, bool) or int(n) != n or not 0 <= n <= count:
        raise ValueError(f'sample_null_pairs: n must be an integer in [0, {count}], got {n!r}')
    return _from_rank(sorted_pos, n_S, _distinct_ranks(count, int(n), pos_pairs.device, generator))


def twin_eval_curve(xS, xT, pos_pairs, thresholds):
    """(nFN, nFP): int64 tensors (T,) on the features' device for up to 16 thresholds (Python numbers): nFN[t] = the positive
    pairs (as listed, duplicates included, like TwinEval) with d2 > thresholds[t], nFP[t] = the null pairs -- the whole
    complement of the distinct positives -- with d2 < thresholds[t].  One dense pass over all n_T * n_S pairs
    (fieldconv_amd.losses.twin_count_dense) minus the positives' part, exact because both use the same d2 bits."""
    from ..losses import pair_sqdist, twin_count_dense
    below, _ = twin_count_dense(xS, xT, thresholds)
    n_T, n_S = int(xT.shape[0]), int(xS.shape[0])
    lin = _sorted_positive_index(pos_pairs, n_T, n_S, 'twin_eval_curve')
    distinct = torch.stack((torch.div(lin, n_S, rounding_mode='floor'), lin % n_S), 1)
    thr = torch.tensor([float(t) for t in thresholds], dtype=xS.dtype, device=xS.device)
    d_listed = pair_sqdist(xS, xT, pos_pairs)
    d_distinct = pair_sqdist(xS, xT, distinct)
    n_fn = (d_listed[None, :] > thr[:, None]).sum(1)
    n_fp = below - (d_distinct[None, :] < thr[:, None]).sum(1)
    return n_fn, n_fp


def hard_null_pairs(xS, xT, pos_pairs, per_row=1):
    """(R * per_row, 2) int64 hard negatives: for each distinct xT row a of pos_pairs, in ascending order, the per_row (1..8)
    rows of xS nearest to xT[a] that are not a's positive, nearest first -- the non-matching pairs a descriptor confuses most,
    where a uniform draw (sample_null_pairs) is almost always already far apart.  One match_descriptors call with the positives
    excluded (fieldconv_amd.matching; the losses' d2, ties to the lower row).  A row with more than one distinct positive raises
    ValueError.  Slots without a candidate (xS has fewer than per_row + 1 rows, NaN features) are dropped, so fewer rows can
    come back; the result is a valid n_ for twin_loss.  The positives are checked and the row count is read back on the host."""
    from ..matching import match_descriptors
    if not torch.is_tensor(xS) or not torch.is_tensor(xT) or xS.dim() != 2 or xT.dim() != 2:
        raise ValueError('hard_null_pairs: xS and xT must be (N,C) tensors')
    n_T, n_S = int(xT.shape[0]), int(xS.shape[0])
    lin = _sorted_positive_index(pos_pairs, n_T, n_S, 'hard_null_pairs')
    rows, true_row = torch.div(lin, n_S, rounding_mode='floor'), lin % n_S
    if rows.numel() > 1 and bool((rows[1:] == rows[:-1]).any()):
        raise ValueError('hard_null_pairs: a row of xT has more than one distinct positive (one row of xS can be excluded per row)')
    exclude = torch.full((n_T,), -1, dtype=torch.int64, device=pos_pairs.device)
    exclude[rows] = true_row
    idx, _ = match_descriptors(xS, xT, k=per_row, exclude=exclude)
    near = idx[rows]                                                    # (R, per_row), nearest first
    pairs = torch.stack((rows[:, None].expand_as(near), near), 2).reshape(-1, 2)
    return pairs[pairs[:, 1] >= 0]
