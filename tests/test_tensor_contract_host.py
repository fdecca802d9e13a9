"""Every operator takes its tensors BY VALUE: whatever a launch takes the address of is contiguous and carries neither the lazy conjugate
nor the lazy negative bit -- the kernels read raw memory, and `x.conj().contiguous()` is `x.conj()` itself, the bit still set and the
un-conjugated memory behind it.

No GPU here: the real library with every enqueueing entry point stubbed (test_host_logic._CountingLibrary), the device guards patched
away, the Python autograd nodes (FIELDCONV_CPP_NODES=0).  Every `data_ptr()` taken by the package's own code is checked; every public
operator is driven once forward and once through torch.autograd.grad with each FORM of each tensor argument and of the cotangent.  A form
has the value of the plain tensor and another representation."""
import ctypes
import os
import re
import sys

import pytest
import torch

from conftest import ROOT
from oracle.torch_composites import FCPrecomp
from test_host_logic import _CountingLibrary

import fieldconv_amd
from fieldconv_amd import _launch, _lib

PKG = os.path.dirname(os.path.abspath(fieldconv_amd.__file__))
# not launch operands: cache keys made of an address (functional._tkey), the alignment test of by_value itself (made on the resolved tensor)
EXEMPT = {'_tkey', 'by_value'}


# ------------------------------------------------------------------------------------------------------------------------- forms
def lazy_conj(t):
    return t.conj().resolve_conj().conj()


def lazy_neg(t):
    return torch.complex(torch.zeros_like(t), -t).conj().imag


def dense_neg(t):
    # The bit on a CONTIGUOUS tensor -- the one form on which a bare .contiguous() keeps it (the imaginary part above is strided as well,
    # so any copy resolves it).  torch._neg_view is torch's own, undocumented, way to make one (its test suite uses it for the same
    # purpose); the tests accept that dependency for the sake of the case, the package does not use it.
    return torch._neg_view(-t)


def transposed(t):
    return t.transpose(0, -1).contiguous().transpose(0, -1)


def every_other(t):
    wide = torch.zeros(*t.shape[:-1], 2 * t.shape[-1], dtype=t.dtype, device=t.device)
    wide[..., ::2] = t
    return wide[..., ::2]


def offset_view(t):
    flat = torch.zeros(t.numel() + 3, dtype=t.dtype, device=t.device)
    flat[1:1 + t.numel()] = t.reshape(-1)
    return flat[1:1 + t.numel()].view(t.shape)


def expanded_row(t):
    return t[:1].expand(t.shape)          # (cotangents: what .sum() sends back; the value is that of the first row, repeated)


def forms_of(t, cotangent=False):
    """{name: tensor of t's value in another representation}; a stride-0 expand (cotangents only) has the value of its first row"""
    out = {'lazy_conj': lazy_conj(t)} if t.is_complex() else {'lazy_neg': lazy_neg(t), 'dense_neg': dense_neg(t)}
    if t.dim() >= 2 and t.shape[0] > 1 and t.shape[-1] > 1:
        out['transposed'] = transposed(t)
    if t.dim() >= 1 and t.shape[-1] > 1:
        out['every_other'] = every_other(t)
    out['offset'] = offset_view(t)
    if cotangent and t.dim() >= 1 and t.shape[0] > 1:
        out['expanded'] = expanded_row(t)
    return out


def test_forms_keep_the_value_and_change_the_representation():
    torch.manual_seed(0)
    z, r = torch.randn(5, 6, dtype=torch.complex64), torch.randn(5, 6)
    assert lazy_conj(z).is_conj() and lazy_conj(z).contiguous().is_conj() and lazy_conj(z).contiguous().data_ptr() != z.data_ptr()
    assert lazy_neg(r).is_neg()          # (the imaginary part of a complex tensor: strided as well)
    assert dense_neg(r).is_contiguous() and dense_neg(r).contiguous().is_neg()
    for t in (z, r):
        for name, f in forms_of(t).items():
            assert torch.equal(f, t), name
            assert f.is_conj() or f.is_neg() or not f.is_contiguous() or f.data_ptr() % 16 != 0, name
    assert offset_view(z).is_contiguous() and offset_view(z).data_ptr() % 16 == 8
    assert offset_view(r).is_contiguous() and offset_view(r).data_ptr() % 8 == 4


def test_the_helper_returns_a_plain_tensor_itself():
    torch.manual_seed(0)
    for t in (torch.randn(4, 3), torch.randn(4, 3, dtype=torch.complex64), torch.randn(7, dtype=torch.float64), torch.empty(0, 3)):
        assert _launch.by_value(t) is t
        assert _launch.by_value(t, 16) is t               # (a fresh allocation is aligned)
    z = torch.randn(4, 6, dtype=torch.complex64)
    for name, f in forms_of(z, cotangent=True).items():
        got = _launch.by_value(f, 16)
        assert got is not f, name
        assert got.is_contiguous() and not got.is_conj() and not got.is_neg() and got.data_ptr() % 16 == 0, name
        assert torch.equal(got, f), name
    off = offset_view(z)
    assert _launch.by_value(off) is off                   # contiguous, no bits: element-wise kernels read it in place
    r = torch.randn(4, 6)
    assert _launch.by_value(offset_view(r), 8).data_ptr() % 8 == 0 and _launch.by_value(offset_view(r)) is not None
    # every module binds the one helper
    from fieldconv_amd import dropout, functional, head, losses, matching, norm, pooling, transfer
    for mod in (dropout, functional, head, losses, matching, norm, pooling, transfer):
        assert mod._by_value is _launch.by_value, mod.__name__


# ------------------------------------------------------------------------------------------------------ the stubbed library, checked
class _Checker:
    def __init__(self):
        self.taken, self.bad = 0, []

    def check(self, t, where):
        self.taken += 1
        if t.is_conj() or t.is_neg() or not t.is_contiguous():
            self.bad.append(f'{where}: {tuple(t.shape)} {t.dtype} stride {tuple(t.stride())} conj={t.is_conj()} neg={t.is_neg()}')


@pytest.fixture
def host(monkeypatch):
    """The package bound to a stubbed library on CPU tensors; -> the _Checker that sees every address the package's code takes"""
    from fieldconv_amd import functional, losses, matching, transfer
    header = open(os.path.join(ROOT, 'include', 'fieldconv_hip.h')).read()
    counting = _CountingLibrary(_lib.load(), header)
    # (every declaration with a stream parameter, wherever a comment in front of it names a function)
    counting.enqueue |= {m.group(1) for m in re.finditer(r'^\w[\w \*]*?\b(fc_[a-z0-9_]+)\s*\(([^;{}]*)\);', header, flags=re.M)
                         if re.search(r'void\*\s*stream\b', m.group(2))}
    monkeypatch.setattr(_lib, 'load', lambda path=None: counting)
    monkeypatch.setattr(functional, 'on_device', lambda t: True)
    monkeypatch.setattr(functional, '_require_device', lambda t, what: None)
    for mod in ('functional', 'pooling', 'losses', 'matching', 'head', 'transfer', 'norm', 'dropout'):
        m = getattr(fieldconv_amd, mod, None) or __import__('fieldconv_amd.' + mod, fromlist=[mod])
        monkeypatch.setattr(m, '_on', lambda device: functional._NO_GUARD)
        monkeypatch.setattr(m, '_stream', lambda: ctypes.c_void_p(0))
    monkeypatch.setattr(losses, '_features', lambda xS, xT, what: None)
    monkeypatch.setattr(matching, '_features', lambda xS, xT, what: None)
    monkeypatch.setattr(transfer, '_device_of', lambda t, family: t.device)
    for name in ('FIELDCONV_BLOCK_CALLS', 'FIELDCONV_NO_FUSED_EPILOGUE', 'FIELDCONV_NO_EDGE_SPLIT', 'FIELDCONV_ECHO_TAIL'):
        monkeypatch.delenv(name, raising=False)
    monkeypatch.setenv('FIELDCONV_CPP_NODES', '0')
    checker = _Checker()
    real = torch.Tensor.data_ptr

    def data_ptr(t):
        f = sys._getframe(1)
        if f.f_code.co_filename.startswith(PKG) and f.f_code.co_name not in EXEMPT:
            g = f.f_back if f.f_code.co_filename == _launch.__file__ else f          # (an idiom of _launch: name its caller)
            checker.check(t, f'{os.path.basename(g.f_code.co_filename)}:{g.f_lineno} {g.f_code.co_name}')
        return real(t)
    monkeypatch.setattr(torch.Tensor, 'data_ptr', data_ptr)
    # the pointer idioms the modules bind go through the same check (they call data_ptr from _launch.py)
    assert functional._p.__module__ == _launch.__name__ and functional._po is _launch._po and functional._dp is _launch._dp
    return checker


def test_the_checker_sees_a_raw_read(host):
    from fieldconv_amd import functional
    z = torch.randn(3, 2, dtype=torch.complex64)
    functional._p(z), functional._po(z), functional._dp(z), _launch.ptr(z)
    assert host.taken == 4 and not host.bad
    functional._p(lazy_conj(z)), _launch.ptr(lazy_neg(z.real)), functional._dp(transposed(z))
    assert len(host.bad) == 3


def _drive(host, name, fn, args, out_index=None):
    """fn(*args) -> tensor (or tuple: out_index); args: leaf tensors.  Forward and autograd.grad for every form of every argument and of the
    cotangent, and once with the cotangent's bit coming from the graph itself (a .conj() consumer).  -> the violations, by case"""
    failures = {}

    def run(case, call_args, cot=None, through_conj=False):
        host.bad.clear()
        before = host.taken
        leaves = [a.detach().requires_grad_(a.is_floating_point() or a.is_complex()) for a in args]
        fed = [form(leaf) if form is not None else leaf for leaf, form in zip(leaves, call_args)]
        y = fn(*fed)
        y = y if out_index is None else y[out_index]
        wanted = [leaf for leaf in leaves if leaf.requires_grad]
        if y.requires_grad:
            g = torch.randn(y.shape, dtype=y.dtype) if cot is None else cot(torch.randn(y.shape, dtype=y.dtype))
            torch.autograd.grad(y.conj() if through_conj else y, wanted, grad_outputs=g, allow_unused=True)
        assert host.taken > before, (name, case)
        if host.bad:
            failures[case] = list(host.bad)

    run('plain', [None] * len(args))
    FORMS = {'lazy_conj': lazy_conj, 'lazy_neg': lazy_neg, 'dense_neg': dense_neg, 'transposed': transposed, 'every_other': every_other, 'offset': offset_view,
             'expanded': expanded_row}
    for i, a in enumerate(args):
        for fname in forms_of(a):
            run(f'arg{i}:{fname}', [FORMS[fname] if j == i else None for j in range(len(args))])
    leaves = [a.detach() for a in args]
    with torch.no_grad():
        y = fn(*leaves)
    y = y if out_index is None else y[out_index]
    if not (y.is_floating_point() or y.is_complex()):
        return failures
    for fname in forms_of(y, cotangent=True):
        run(f'cotangent:{fname}', [None] * len(args), cot=FORMS[fname])
    if y.is_complex():
        run('cotangent:conj_in_graph', [None] * len(args), through_conj=True)
    return failures


# ------------------------------------------------------------------------------------------------------------------- the operators
def _mesh(N=40, k=8, B=2, R=6, dtype=torch.float32):
    from fieldconv_amd.data import sphere_support
    data = sphere_support(N, k)
    edges, sten, ln, wxp = FCPrecomp(B, R, data.epsilon)(data)
    if dtype == torch.float64:
        sten, ln, wxp = sten.to(torch.complex128), ln.to(torch.float64) if not ln.is_complex() else ln.to(torch.complex128), wxp.to(torch.complex128)
    return N, edges, sten, ln, wxp


def _operators():
    """{name: (fn, args, out_index)} -- every public operator, each kernel family of the convolution once"""
    from fieldconv_amd import blocks, dropout, functional as Fn, head, losses, matching, norm, pooling, transfer
    from fieldconv_amd.graph import get_edge_csr, get_graph
    torch.manual_seed(0)
    B, R = 2, 6
    N, edges, sten, ln, wxp = _mesh(B=B, R=R)
    graph = get_graph(edges, sten, N)
    F = 2 * B + 1
    cx = lambda *s: torch.randn(*s, dtype=torch.complex64)
    I, O = 5, 6
    x, w_eff = cx(N, I), cx(O, I, R, F)
    zonal, sph, phase = torch.randn(O, I, R), torch.randn(O, I, R, B, 2), torch.randn(O, I, B + 1)
    zonal2, sph2 = torch.randn(O, I, R, 2), torch.randn(O, I, R, 2 * B, 2)
    bias = torch.rand(O)
    ops = {}
    ops['field_conv'] = (lambda x, w: Fn.field_conv(x, w, graph), [x, w_eff], None)
    for ftype in (0, 1):
        ops[f'field_conv_params[{ftype}]'] = (lambda x, z, s, p, ftype=ftype: Fn.field_conv_params(x, z, s, p, ftype, B, graph), [x, zonal, sph, phase], None)
    ops['field_conv_params[2]'] = (lambda x, z, s, p: Fn.field_conv_params(x, z, s, p, 2, B, graph), [x, zonal2, sph2, phase], None)
    ops['field_conv_act'] = (lambda x, z, s, p, b, a: Fn.field_conv_act(x, z, s, p, 1, B, graph, b, a), [x, zonal, sph, phase, bias, cx(N, O)], None)
    Iw = 70                                                                # more than one channel block
    ops['field_conv wide'] = (lambda x, w: Fn.field_conv(x, w, graph), [cx(N, Iw), cx(O, Iw, R, F)], None)
    ops['field_conv_params wide'] = (lambda x, z, s, p: Fn.field_conv_params(x, z, s, p, 1, B, graph),
                                     [cx(N, Iw), torch.randn(O, Iw, R), torch.randn(O, Iw, R, B, 2), torch.randn(O, Iw, B + 1)], None)
    xd, wd = x.to(torch.complex128), w_eff.to(torch.complex128)
    graph_d = get_graph(edges, sten.to(torch.complex128), N)
    ops['field_conv run-time'] = (lambda x, w: Fn.field_conv(x, w, graph_d), [xd, wd], None)
    re_w, im_w = torch.randn(O, I), torch.randn(O, I)
    ops['tangent_lin'] = (Fn.tangent_lin, [x, re_w, im_w], None)
    ops['tangent_lin gemm'] = (Fn.tangent_lin, [xd, re_w.double(), im_w.double()], None)
    ops['tangent_nonlin'] = (Fn.tangent_nonlin, [x, torch.rand(I)], None)
    ops['tangent_nonlin f64'] = (Fn.tangent_nonlin, [xd, torch.rand(I, dtype=torch.float64)], None)
    ops['soft_abs'] = (Fn.soft_abs, [x], None)
    ops['echo_descriptors'] = (lambda x: Fn.echo_descriptors(x, edges, ln, wxp, 3), [x], None)
    ops['echo_descriptors generic'] = (lambda x: Fn.echo_descriptors(x, edges, ln, wxp, 9), [x], None)
    lift = sten[..., B:B + 2]
    za, zm, ph = torch.randn(O, 3, R), torch.randn(O, 3, R), torch.randn(O, 3)
    xr = torch.randn(N, 3)
    ops['trans_field'] = (lambda x, s, a, m, p: Fn.trans_field(x, edges, s, a, m, p, 1), [xr, lift.contiguous(), za, zm, ph], None)
    ops['trans_field generic'] = (lambda x, s, a, m, p: Fn.trans_field(x, edges, s, a, m, p, 1),
                                  [xr.double(), lift.contiguous().to(torch.complex128), za.double(), zm.double(), ph.double()], None)
    # the block-level entry points, Python nodes
    C = 6
    z1, s1, p1 = torch.randn(C, C, R), torch.randn(C, C, R, B, 2), torch.randn(C, C, B + 1)
    ops['resnet_block'] = (lambda x, z1, s1, p1, b1, z2, s2, p2, b2, re, im: blocks._ResnetBlockFn.apply(x, z1, s1, p1, b1, z2, s2, p2, b2, re, im, 1, B, graph),
                           [cx(N, C), z1, s1, p1, torch.rand(C), z1 + 1, s1 + 1, p1 + 1, torch.rand(C), torch.randn(C, C), torch.randn(C, C)], None)
    slots = Fn.echo_slot_order(graph, ln, wxp)
    ops['echo_block'] = (lambda x, z, s, p, b: blocks._EchoBlockFn.apply(x, z, s, p, b, 1, B, C, 3, graph, slots), [cx(N, C), z1, s1, p1, torch.rand(C)], None)
    dS = int(_lib.load().fc_echo_hist_dim(3))
    D, H1, H2, Q = C * dS, 16, 8, 4
    head_args = [torch.randn(N, D), cx(N, C), torch.randn(H1, D), torch.randn(H1), torch.randn(H2, H1), torch.randn(H2), torch.randn(Q, H2), torch.randn(Q),
                 torch.randn(Q, C), torch.randn(Q)]
    ops['echo_head'] = (blocks._EchoHeadFn.apply, head_args, None)
    ops['echo_tail'] = (blocks._EchoTailFn.apply, head_args[:2] + [t.clone() for t in head_args[2:]], None)
    csr = get_edge_csr(edges, N)
    sten_l, stride = Fn._TransFieldFn._stencil(lift.contiguous())          # (a (E,R,2) VIEW of the full stencil is read in place, by design)
    ops['lift_block'] = (lambda x, a, m, p, b: blocks._LiftBlockFn.apply(x, sten_l, stride, a, m, p, b, 1, csr), [xr, za, zm, ph, torch.rand(O)], None)
    assert sten_l.is_contiguous() and stride == 2
    # pooling, losses, matching, head
    ptr = torch.tensor([0, 17, 17, N])
    ops['mesh_pool softabs'] = (lambda x: pooling._MeshPool.apply(x, ptr, 0, True), [x], None)
    ops['mesh_pool real sum'] = (lambda x: pooling._MeshPool.apply(x, ptr, 1, False), [xr], None)
    ops['mesh_max'] = (lambda x: pooling._MeshMax.apply(x, ptr), [x], 0)
    xS, xT = torch.randn(9, 4), torch.randn(7, 4)
    p_, n_ = torch.tensor([[0, 1], [2, 3], [6, 8]]), torch.tensor([[1, 1], [3, 0]])
    ops['twin_loss'] = (lambda s, t, y: losses.twin_loss(s, t, p_, n_, y), [xS, xT, torch.rand(2)], None)
    ops['pair_sqdist'] = (lambda s, t: losses.pair_sqdist(s, t, p_), [xS, xT], None)
    ops['twin_count_dense'] = (lambda s, t: losses.twin_count_dense(s, t, [1.0])[0], [xS, xT], None)
    tgt = torch.randint(0, 4, (9,))
    ops['label_smoothing_loss'] = (lambda p, w: losses._LabelSmoothing.apply(p, tgt, w, 0.9, 0.1 / 3), [xS, torch.rand(4)], None)
    ops['match_descriptors'] = (lambda s, t: matching.match_descriptors(s, t, 2)[1], [xS, xT], None)
    hw, hb = torch.randn(5, 4), torch.randn(5)
    htgt = torch.randint(0, 5, (9,))
    for red in ('none', 'sum', 'mean'):
        ops[f'linear_cross_entropy[{red}]'] = (lambda g, red=red: head._LinearCrossEntropy.apply(xS.detach().requires_grad_(True) * 1 + 0 * g.sum(), hw, hb, htgt, red, 0.9, 0.025, -100, 0),
                                               [torch.zeros(1)], None)
    # transfer, norm, dropout
    rows = torch.tensor([[0, 1], [0, 2], [1, 0], [2, 3], [2, 1]])
    plan = transfer.TransferPlan(rows, torch.rand(5), torch.randn(5, dtype=torch.complex64), n_out=3, n_in=4)
    ops['tangent_transfer'] = (lambda x: transfer._TangentTransfer.apply(x, plan), [cx(4, 3)], None)
    ops['tangent_transfer_max'] = (lambda x: transfer._TangentTransferMax.apply(x, plan), [cx(4, 3)], 0)
    ops['tangent_norm'] = (lambda x, g, w: norm._TangentNorm.apply(x, g, ptr, w, 1e-5), [x, torch.rand(I), torch.rand(N)], None)
    ops['tangent_dropout'] = (lambda x: dropout._TangentDropout.apply(x, ptr, 3, dropout.drop_threshold(0.25), dropout.keep_scale(0.25), 7, 0, None, 0), [x], None)
    return ops


def _names():
    return ['field_conv', 'field_conv_params[0]', 'field_conv_params[1]', 'field_conv_params[2]', 'field_conv_act', 'field_conv wide',
            'field_conv_params wide', 'field_conv run-time', 'tangent_lin', 'tangent_lin gemm', 'tangent_nonlin', 'tangent_nonlin f64', 'soft_abs',
            'echo_descriptors', 'echo_descriptors generic', 'trans_field', 'trans_field generic', 'resnet_block', 'echo_block', 'echo_head',
            'echo_tail', 'lift_block', 'mesh_pool softabs', 'mesh_pool real sum', 'mesh_max', 'twin_loss', 'pair_sqdist', 'twin_count_dense',
            'label_smoothing_loss', 'match_descriptors', 'linear_cross_entropy[none]', 'linear_cross_entropy[sum]', 'linear_cross_entropy[mean]',
            'tangent_transfer', 'tangent_transfer_max', 'tangent_norm', 'tangent_dropout']


def test_every_operator_is_listed(host):
    assert sorted(_operators()) == sorted(_names())


@pytest.mark.parametrize('name', _names())
def test_operator_takes_its_tensors_by_value(host, name):
    """No launch of `name`, forward or backward, takes the address of a tensor that is non-contiguous or carries a lazy bit, whatever
    the form of its arguments and of the cotangent."""
    fn, args, out_index = _operators()[name]
    failures = _drive(host, name, fn, args, out_index)
    assert not failures, '\n'.join(f'{case}: {bad}' for case, bads in failures.items() for bad in bads)


def test_the_head_refuses_what_it_would_read_raw(host):
    from fieldconv_amd import head
    h, w, b = torch.randn(6, 4), torch.randn(5, 4), torch.randn(5)
    tgt = torch.randint(0, 5, (6,))
    for bad in (lazy_neg(h), transposed(h)):
        with pytest.raises(ValueError, match='not contiguous'):
            head.linear_cross_entropy(bad, w, b, tgt)
    for args in ((dense_neg(h), w, b), (h, dense_neg(w), b), (h, w, dense_neg(b))):
        with pytest.raises(ValueError, match='lazy negative'):
            head.linear_cross_entropy(*args, tgt)
    assert host.taken == 0


def test_effective_filter_takes_its_parameters_by_value():
    """the run-time path assembles the filter in torch (nn/field_conv.py): view_as_complex refuses a strided pair axis, an odd storage
    offset and a lazy negative, so the pairs are copied first; values and gradients are those of the plain tensors"""
    from fieldconv_amd.nn.field_conv import effective_filter
    torch.manual_seed(0)
    B = 2
    for ftype, z, s in ((1, torch.randn(3, 2, 4), torch.randn(3, 2, 4, B, 2)), (2, torch.randn(3, 2, 4, 2), torch.randn(3, 2, 4, 2 * B, 2))):
        p = torch.randn(3, 2, B + 1)
        leaves = [t.clone().requires_grad_(True) for t in (z, s, p)]
        w = effective_filter(*leaves, ftype, B)
        g = torch.randn(w.shape, dtype=w.dtype)
        want = torch.autograd.grad(w, leaves, g, allow_unused=True)
        for i in range(3):
            for name, form in (('lazy_neg', lazy_neg), ('dense_neg', dense_neg), ('transposed', transposed), ('every_other', every_other),
                               ('offset', offset_view)):
                fed = [form(t) if j == i else t for j, t in enumerate(leaves)]
                w2 = effective_filter(*fed, ftype, B)
                assert torch.equal(w2, w), (ftype, i, name)
                got = torch.autograd.grad(w2, leaves, g, allow_unused=True)
                assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(got, want)), (ftype, i, name)
