"""Host-side tests of the losses (TwinLoss, TwinEval, LabelSmoothingLoss) and the pair utilities: the public surface, argument
checks, the index arithmetic of the null pairs against np.setdiff1d, and the consistency of tests/golden/losses.npz (made from the
reference's modules by tests/golden/make_golden_losses.py) with the float64 numpy restatements the GPU tests reuse."""
import inspect

import numpy as np
import pytest
import torch

import _losses_ref as ref
from conftest import load_golden, rel_err


def test_names_import_and_defaults():
    import fieldconv_amd.nn as fnn
    from fieldconv_amd.nn import LabelSmoothingLoss, TwinEval, TwinLoss
    assert {'TwinLoss', 'TwinEval', 'LabelSmoothingLoss'} <= set(fnn.__all__)
    assert all(isinstance(n, str) and hasattr(fnn, n) for n in fnn.__all__)

    def defaults(cls):
        return [(p.name, p.default) for p in list(inspect.signature(cls.__init__).parameters.values())[1:]]
    assert defaults(TwinLoss) == [('mu', 5)]
    assert defaults(TwinEval) == [('mu', 5), ('ratio', 0.5)]
    assert defaults(LabelSmoothingLoss) == [('classes', inspect.Parameter.empty), ('smoothing', 0.0), ('dim', -1), ('weight', None)]
    for m in (TwinLoss(), TwinEval(), LabelSmoothingLoss(8, smoothing=0.2, dim=1)):
        assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())
    ls = LabelSmoothingLoss(8, smoothing=0.2, dim=1)
    assert (ls.cls, ls.smoothing, ls.dim, ls.weight) == (8, 0.2, 1, None) and abs(ls.confidence - 0.8) < 1e-15


def test_functional_forms_and_utils_exported():
    from fieldconv_amd import losses, utils
    for name in ('twin_loss', 'pair_sqdist', 'label_smoothing_loss', 'twin_count_dense', 'twin_eval'):
        assert callable(getattr(losses, name))
    for name in ('null_pair_count', 'null_pairs_from_rank', 'sample_null_pairs', 'twin_eval_curve'):
        assert callable(getattr(utils, name)) and name in utils.__all__


def test_cpu_tensors_raise():
    from fieldconv_amd import losses
    from fieldconv_amd.nn import LabelSmoothingLoss, TwinEval, TwinLoss
    xS, xT = torch.rand(10, 16), torch.rand(12, 16)
    p = torch.tensor([[0, 1], [2, 3]])
    with pytest.raises(RuntimeError, match='no CPU path'):
        TwinLoss()(xS, xT, p, p)
    with pytest.raises(RuntimeError, match='no CPU path'):
        TwinEval()(xS, xT, p, p)
    with pytest.raises(RuntimeError, match='no CPU path'):
        losses.pair_sqdist(xS, xT, p)
    with pytest.raises(RuntimeError, match='no CPU path'):
        losses.twin_count_dense(xS, xT, [1.0])
    with pytest.raises(RuntimeError, match='no CPU path'):
        LabelSmoothingLoss(8)(torch.randn(4, 8), torch.zeros(4, dtype=torch.int64))


def test_bad_arguments_raise():
    from fieldconv_amd import losses, utils
    from fieldconv_amd.nn import LabelSmoothingLoss
    for s in (-0.1, 1.0, 1.5):
        with pytest.raises(ValueError):
            LabelSmoothingLoss(8, smoothing=s)
    for d in (0, 2, -2):
        with pytest.raises(ValueError):
            LabelSmoothingLoss(8, dim=d)
    with pytest.raises(ValueError):
        LabelSmoothingLoss(1)
    with pytest.raises(ValueError):
        LabelSmoothingLoss(8)(torch.randn(2, 3, 8), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError):
        losses.label_smoothing_loss(torch.randn(4, 8).to(torch.float16), torch.zeros(4, dtype=torch.int64), 8)
    # an out-of-range pair index (the utilities take CPU index tensors)
    for bad in ([[0, 53]], [[37, 0]], [[-1, 0]], [[0, -1]]):
        with pytest.raises(IndexError):
            utils.null_pair_count(torch.tensor(bad), 37, 53)
    with pytest.raises(IndexError):
        utils.null_pairs_from_rank(torch.tensor([[0, 0]]), 3, 3, torch.tensor([8]))
    with pytest.raises(ValueError):
        utils.sample_null_pairs(torch.tensor([[0, 0]]), 3, 3, 9)
    with pytest.raises(ValueError):
        utils.null_pair_count(torch.tensor([[0, 0]], dtype=torch.int32), 3, 3)


def _positives(n_T, n_S, P, seed):
    g = torch.Generator().manual_seed(seed)
    pos = torch.stack((torch.randint(0, n_T, (P,), generator=g), torch.randint(0, n_S, (P,), generator=g)), 1)
    return torch.cat((pos, pos[:P // 3], torch.tensor([[0, 0], [n_T - 1, n_S - 1], [0, 1], [0, 2]])))          # duplicates, both ends, a run


def test_null_pairs_from_rank_equals_setdiff():
    from fieldconv_amd.utils import null_pair_count, null_pairs_from_rank
    n_T, n_S = 37, 53
    pos = _positives(n_T, n_S, 200, 0)
    want = np.setdiff1d(np.arange(n_T * n_S), (pos[:, 0] * n_S + pos[:, 1]).numpy())
    count = null_pair_count(pos, n_T, n_S)
    assert count == want.size and count < n_T * n_S - 150
    got = null_pairs_from_rank(pos, n_T, n_S, torch.arange(count))
    assert got.dtype == torch.int64 and tuple(got.shape) == (count, 2)
    assert np.array_equal((got[:, 0] * n_S + got[:, 1]).numpy(), want)
    # no positives at all: the identity
    none = torch.empty((0, 2), dtype=torch.int64)
    assert null_pair_count(none, 4, 5) == 20
    assert np.array_equal(null_pairs_from_rank(none, 4, 5, torch.arange(20)).numpy(), np.stack(np.divmod(np.arange(20), 5), 1))


@pytest.mark.parametrize('n', [0, 1, 512, 1700])
def test_sample_null_pairs(n):
    from fieldconv_amd.utils import null_pair_count, sample_null_pairs
    n_T, n_S = 37, 53
    pos = _positives(n_T, n_S, 200, 1)
    assert n <= null_pair_count(pos, n_T, n_S)
    a = sample_null_pairs(pos, n_T, n_S, n, generator=torch.Generator().manual_seed(5))
    b = sample_null_pairs(pos, n_T, n_S, n, generator=torch.Generator().manual_seed(5))
    c = sample_null_pairs(pos, n_T, n_S, n, generator=torch.Generator().manual_seed(6))
    assert tuple(a.shape) == (n, 2) and a.dtype == torch.int64 and torch.equal(a, b)
    lin = (a[:, 0] * n_S + a[:, 1]).numpy()
    assert np.unique(lin).size == n                                                       # distinct
    assert not np.isin(lin, (pos[:, 0] * n_S + pos[:, 1]).numpy()).any()                  # none positive
    assert n == 0 or (0 <= a.min() and int(a[:, 0].max()) < n_T and int(a[:, 1].max()) < n_S)
    if n >= 512:
        assert not torch.equal(a, c)
        assert not np.array_equal(lin, np.sort(lin))                                      # drawn, not enumerated
    torch.manual_seed(3)
    d = sample_null_pairs(pos, n_T, n_S, n)
    torch.manual_seed(3)
    assert torch.equal(d, sample_null_pairs(pos, n_T, n_S, n))


def test_sample_null_pairs_is_uniform():
    """Every null pair of a small grid is drawn about equally often: 4 000 draws of 5 out of 21, expected 952 each, standard
    deviation 27; the bound is 5 of them."""
    from fieldconv_amd.utils import sample_null_pairs
    pos = torch.tensor([[0, 0], [2, 3], [4, 4], [2, 3]])
    g = torch.Generator().manual_seed(0)
    hits = np.zeros(25, dtype=np.int64)
    for _ in range(4000):
        s = sample_null_pairs(pos, 5, 5, 5, generator=g)
        hits[(s[:, 0] * 5 + s[:, 1]).numpy()] += 1
    assert hits[[0, 13, 24]].sum() == 0
    rest = np.delete(hits, [0, 13, 24])
    assert np.abs(rest - 4000 * 5 / 22).max() < 5 * 27 and rest.sum() == 20000


def test_fixture_twin_matches_restatement():
    """The float64 restatement reproduces the reference's gradients to 1e-12 (float64 run) and its float32 run at float32's
    precision; the reference's loss is a float32 tensor in both runs (it accumulates into torch.empty(1).float()), so the float64
    run's loss is compared after the same two roundings: fl32(fl32(positive part) + fl32(negative part))."""
    cases = load_golden('losses.npz')
    for name in ('twin_n300', 'twin_repeat'):
        c = cases[name]
        assert c['xS'].dtype == np.float32 and c['loss_f64'].dtype == np.float32 and c['gS_f64'].dtype == np.float64
        lp, ln, gS, gT = ref.twin_loss(c['xS'], c['xT'], c['p'], c['n'], c['yN'], float(c['mu']))
        assert rel_err(gS, c['gS_f64']) <= 1e-12 and rel_err(gT, c['gT_f64']) <= 1e-12
        assert rel_err(gS, c['gS_f32']) <= 1e-5 and rel_err(gT, c['gT_f32']) <= 1e-5
        assert np.float32(np.float32(lp) + np.float32(ln)) == c['loss_f64'][0]
        assert rel_err(lp + ln, c['loss_f32']) <= 1e-5
        thr = np.float32(float(c['mu']) * float(c['eval_ratio']))
        dp = ref.sqdist(c['xT'][c['p'][:, 0]], c['xS'][c['p'][:, 1]])
        dn = ref.sqdist(c['xT'][c['n'][:, 0]], c['xS'][c['n'][:, 1]])
        # counts: no distance of these fixtures lies within float32 rounding of the threshold
        assert np.abs(np.concatenate((dp, dn)) - thr).min() > 1e-4
        assert (int((dp > thr).sum()), int((dn < thr).sum())) == (int(c['nFN_f32']), int(c['nFP_f32'])) == (int(c['nFN_f64']), int(c['nFP_f64']))
        assert 0 < int(c['nFN_f32']) < c['p'].shape[0] and 0 < int(c['nFP_f32']) < c['n'].shape[0]
    rep = cases['twin_repeat']
    assert (rep['p'][:, 0] == 5).all() and (rep['n'][:, 0] == 5).all() and np.unique(rep['p'][:, 1]).size <= 4


def test_fixture_label_smoothing_matches_restatement():
    cases = load_golden('losses.npz')
    seen = set()
    for shape in ('ls_1024x8', 'ls_1x30', 'ls_257x40'):
        c = cases[shape]
        for v in c['variants']:
            smoothing, weighted, classes, dt = ref.parse_variant(str(v))
            loss, grad = ref.label_smoothing(c['pred'], c['target'], classes, smoothing, c['weight'] if weighted else None)
            gate = 1e-12 if dt == np.float64 else 1e-5
            assert c[f'gpred_{v}'].dtype == dt
            assert rel_err(loss, c[f'loss_{v}']) <= gate, (shape, v)
            assert rel_err(grad, c[f'gpred_{v}']) <= gate, (shape, v)
            seen.add((smoothing, weighted, dt, classes != c['pred'].shape[1]))
    assert {(0.0, False), (0.1, False), (0.1, True), (0.0, True)} <= {s[:2] for s in seen}
    assert any(s[3] for s in seen) and {np.float32, np.float64} == {s[2] for s in seen}
