"""Host-side tests of the fused classification head (fieldconv_amd.head, nn.LinearCrossEntropy): the numpy restatement the GPU
tests compare with (tests/_head_ref.py) pinned to torch on the CPU in float64 and to this package's label-smoothing contract
(tests/_losses_ref.py, tests/golden/losses.npz), the public surface, and the argument checks that need no device."""
import os
import re

import numpy as np
import pytest
import torch

import _head_ref as href
import _losses_ref as lref
from conftest import load_golden, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _case(N, H, K, seed, ignore=(), with_bias=True):
    rng = np.random.default_rng(seed)
    h, W = rng.standard_normal((N, H)), rng.standard_normal((K, H)) * 3.0
    b = rng.standard_normal(K) if with_bias else None
    target = rng.integers(0, K, N)
    target[0], target[-1] = 0, K - 1
    for n in ignore:
        target[n] = -100
    return h, W, b, target


@pytest.mark.parametrize('reduction', ['none', 'mean', 'sum'])
@pytest.mark.parametrize('with_bias', [True, False])
def test_restatement_equals_torch_cross_entropy(reduction, with_bias):
    h, W, b, target = _case(23, 7, 11, 1, ignore=(3, 9), with_bias=with_bias)
    ht, Wt = torch.tensor(h, requires_grad=True), torch.tensor(W, requires_grad=True)
    bt = torch.tensor(b, requires_grad=True) if with_bias else None
    loss_t = torch.nn.functional.cross_entropy(torch.nn.functional.linear(ht, Wt, bt), torch.tensor(target), reduction=reduction)
    rng = np.random.default_rng(2)
    up = rng.standard_normal(23) if reduction == 'none' else 0.7
    grads = torch.autograd.grad(loss_t, [ht, Wt] + ([bt] if with_bias else []), grad_outputs=torch.tensor(up, dtype=torch.float64))
    loss, g_h, g_W, g_b = href.head(h, W, b, target, reduction, upstream=up)
    assert rel_err(np.asarray(loss), loss_t.detach().numpy()) < 1e-13
    assert rel_err(g_h, grads[0].numpy()) < 1e-13 and rel_err(g_W, grads[1].numpy()) < 1e-13
    if with_bias:
        assert rel_err(g_b, grads[2].numpy()) < 1e-13
    if reduction == 'none':
        assert loss[3] == 0 and loss[9] == 0 and (g_h[3] == 0).all()


def test_restatement_ignore_and_bad_targets():
    h, W, b, target = _case(9, 4, 5, 3)
    every = np.full(9, -100)
    assert np.isnan(href.head(h, W, b, every, 'mean')[0]) and href.head(h, W, b, every, 'sum')[0] == 0
    t = torch.nn.functional.cross_entropy(torch.tensor(href.logits(h, W, b)), torch.tensor(every))
    assert bool(torch.isnan(t))
    for bad in (5, -1, 2 ** 40):
        tb = target.copy()
        tb[4] = bad
        rows = href.loss_rows(href.logits(h, W, b), tb)
        assert np.isnan(rows[4]) and np.isfinite(np.delete(rows, 4)).all()
        loss, g_h, g_W, g_b = href.head(h, W, b, tb, 'mean')
        assert np.isnan(loss) and np.isnan(g_h[4]).all() and np.isfinite(np.delete(g_h, 4, 0)).all() and np.isnan(g_W).all() and np.isnan(g_b).all()


@pytest.mark.parametrize('smoothing', [0.1, 0.5])
def test_restatement_equals_label_smoothing_contract(smoothing):
    """on materialised logits, against tests/_losses_ref.py (what LabelSmoothingLoss is held to): the logit gradient G of the
    restatement is its gradient, so g_h = G W, g_W = G^T h, g_b = column sums"""
    h, W, b, target = _case(31, 6, 13, 4)
    z = href.logits(h, W, b)
    loss_ls, G = lref.label_smoothing(z, target, 13, smoothing)
    loss, g_h, g_W, g_b = href.head(h, W, b, target, 'mean', smoothing)
    assert rel_err(np.asarray(loss), np.asarray(loss_ls)) < 1e-13
    assert rel_err(g_h, G @ W) < 1e-13 and rel_err(g_W, G.T @ h) < 1e-13 and rel_err(g_b, G.sum(0)) < 1e-13


def test_restatement_equals_label_smoothing_fixture():
    """tests/golden/losses.npz (captured from the reference's LabelSmoothingLoss): with W = I and b = 0 the head's logits are
    the fixture's pred, and g_h its recorded gradient"""
    cases = load_golden('losses.npz')
    seen = 0
    for shape in ('ls_1024x8', 'ls_1x30', 'ls_257x40'):
        c = cases[shape]
        K = c['pred'].shape[1]
        for v in c['variants']:
            smoothing, weighted, classes, dt = lref.parse_variant(str(v))
            if weighted or classes != K:
                continue
            gate = 1e-12 if dt == np.float64 else 1e-5          # (the recorded values are the reference's float32 run: tests/test_losses_host.py's gate)
            loss, g_h, _, _ = href.head(c['pred'].astype(np.float64), np.eye(K), None, c['target'], 'mean', smoothing)
            assert rel_err(np.asarray(loss), c[f'loss_{v}']) <= gate and rel_err(g_h, c[f'gpred_{v}']) <= gate, (shape, v)
            seen += 1
    assert seen >= 6


def test_restated_topk_order_and_accuracy():
    z = np.array([[1.0, 3.0, 3.0, -np.inf, np.nan], [np.nan, np.nan, 0.0, -0.0, 2.0]], dtype=np.float32)
    idx, zk = href.topk(z, 6)
    assert idx.tolist() == [[1, 2, 0, 3, 4, -1], [4, 2, 3, 0, 1, -1]]
    assert zk[0, :4].tolist() == [3.0, 3.0, 1.0, -np.inf] and np.isnan(zk[0, 4]) and zk[0, 5] == -np.inf and zk.dtype == np.float32
    t = torch.tensor([[5.0, 1.0, 7.0, 7.0], [0.0, 0.0, 0.0, 0.0]], dtype=torch.float64)
    assert np.array_equal(href.topk(t.numpy(), 2)[0][0], torch.topk(t, 2, dim=1).indices.numpy()[0]) and href.topk(t.numpy(), 2)[0][1].tolist() == [0, 1]
    target = np.array([2, -100, 1, 0])
    idx = np.array([[2, 0], [1, 0], [0, 1], [3, 2]])
    assert href.accuracy(idx, target).tolist() == [1 / 3, 2 / 3]
    from fieldconv_amd.nn import vertex_accuracy
    acc = vertex_accuracy(torch.tensor(idx), torch.tensor(target))
    assert acc.dtype == torch.float64 and np.array_equal(acc.numpy(), href.accuracy(idx, target))
    with pytest.raises(ValueError):
        vertex_accuracy(torch.tensor(idx), torch.tensor(target[:3]))
    with pytest.raises(ValueError):
        vertex_accuracy(torch.tensor(idx).to(torch.int32), torch.tensor(target))


def test_names_exported_and_module_is_a_linear():
    from fieldconv_amd import functional, head, nn
    for name in ('linear_cross_entropy', 'linear_topk', 'linear_logsumexp', 'vertex_accuracy'):
        assert getattr(functional, name) is getattr(head, name)
    assert nn.vertex_accuracy is head.vertex_accuracy and 'LinearCrossEntropy' in nn.__all__ and 'vertex_accuracy' in nn.__all__
    torch.manual_seed(0)
    lin2 = torch.nn.Linear(256, 37)
    torch.manual_seed(0)
    m = nn.LinearCrossEntropy(256, 37, smoothing=0.1)
    assert torch.equal(m.weight, lin2.weight) and torch.equal(m.bias, lin2.bias)          # nn.Linear's names and initialisation
    m.load_state_dict(torch.nn.Linear(256, 37).state_dict())                              # the reference's lin2 loads
    assert [n for n, _ in m.named_parameters()] == ['weight', 'bias']
    assert nn.LinearCrossEntropy(5, 3, bias=False).bias is None
    with pytest.raises(RuntimeError, match='no CPU path'):
        m(torch.randn(4, 256), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(RuntimeError, match='no CPU path'):
        m.predict(torch.randn(4, 256))


def test_bad_arguments_raise():
    from fieldconv_amd.functional import linear_cross_entropy, linear_topk
    from fieldconv_amd.matching import MAX_K
    h, W, b, t = torch.randn(6, 5), torch.randn(4, 5), torch.randn(4), torch.zeros(6, dtype=torch.int64)
    with pytest.raises(RuntimeError, match='no CPU path'):
        linear_cross_entropy(h, W, b, t)
    with pytest.raises(RuntimeError, match='no CPU path'):
        linear_topk(h, W, None)
    with pytest.raises(TypeError, match='float32 only'):
        linear_cross_entropy(h.double(), W.double(), b.double(), t)
    with pytest.raises(TypeError, match='float32 only'):
        linear_topk(h, W.double(), b)
    with pytest.raises(ValueError, match='not contiguous'):
        linear_cross_entropy(torch.randn(5, 6).t(), W, b, t)
    with pytest.raises(ValueError, match='not contiguous'):
        linear_topk(h, torch.randn(4, 10)[:, ::2], b)
    for bad_W, bad_b in ((torch.randn(4, 6), b), (W, torch.randn(5)), (W[0], b), (W, b[:, None])):
        with pytest.raises(ValueError):
            linear_cross_entropy(h, bad_W, bad_b, t)
    assert MAX_K == 8
    for k in (0, MAX_K + 1, 1.5, True):
        with pytest.raises(ValueError, match='k must be'):
            linear_topk(h, W, b, k=k)
    for parts in (-1, 65, 2.0):
        with pytest.raises(ValueError, match='parts must be'):
            linear_cross_entropy(h, W, b, t, parts=parts)
        with pytest.raises(ValueError, match='parts must be'):
            linear_topk(h, W, b, parts=parts)
    with pytest.raises(ValueError, match='reduction'):
        linear_cross_entropy(h, W, b, t, reduction='batchmean')
    for s in (-0.1, 1.0):
        with pytest.raises(ValueError, match='smoothing'):
            linear_cross_entropy(h, W, b, t, smoothing=s)
    with pytest.raises(ValueError, match='two classes'):
        linear_cross_entropy(h, W[:1], b[:1], t, smoothing=0.1)


def test_symbols_declared_and_bound():
    from fieldconv_amd import _lib
    from fieldconv_amd.build import SOURCES
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    declared = set(re.findall(r'\b(fc_[a-z0-9_]+)\s*\(', header))
    names = {'fc_linear_ce_workspace_bytes', 'fc_linear_ce_forward', 'fc_linear_topk', 'fc_linear_ce_backward_input',
             'fc_linear_ce_backward_weight'}
    assert names <= declared and names <= set(_lib.SIGNATURES) and 'fc_linear_ce.hip' in SOURCES
    lib = _lib.load(__import__('fieldconv_amd.build', fromlist=['build_native']).build_native())
    assert lib.fc_abi_version() == 11
    # the workspace query, on the host: O(N parts) forward, nothing for an unsplit weight pass, 0 for arguments out of range
    q = lib.fc_linear_ce_workspace_bytes
    assert q(4999, 256, 4999, 1, 0, 0) == 4999 * 16 + (256 - 4999 * 16 % 256) % 256 and q(4999, 256, 4999, 1, 1, 0) == 0
    assert q(4999, 256, 4999, 3, 0, 0) >= 3 * 4999 * 16 and q(4999, 256, 4999, 0, 0, 0) <= 64 * 4999 * 16 + 256
    assert q(4999, 256, 4999, 3, 1, 0) >= 3 * 4999 * 257 * 4 and q(10, 4, 3, 2, 2, 8) >= 2 * 10 * 8 * 8
    assert q(0, 256, 10, 1, 0, 0) == 0 and q(10, 256, 10, 65, 0, 0) == 0 and q(10, 4, 3, 1, 2, 9) == 0 and q(10, 4, 3, 1, 7, 1) == 0
