"""The tensor contract on the device: op(form(t)) is the operator on the VALUE of form(t), for every form of tests/
test_tensor_contract_host.py, every tensor argument and the cotangent.  One table row per operator: its smallest existing case, the
float64 / complex128 restatement of its own test, that test's measure and gate (imported).  Two assertions per (row, argument, form):

  against the reference   every output and gradient within the gate of the reference on the form's value; for a lazy conjugate the
                          reference itself must move by more than 100 gates when the argument is conjugated (a condition on the inputs:
                          a kernel that ignores the bit cannot pass)
  against the plain form  the operator on a plain copy of the same value is run twice; if those agree bit for bit the form's result
                          equals them bit for bit (the same kernel on the same values).  Every row here is run-to-run reproducible --
                          the test asserts it -- so the comparison is made for all of them.

The block-level entry points have no float64 restatement in the suite: their reference is the one their own test uses, the same module
composed of per-operator nodes (FIELDCONV_BLOCK_CALLS=0) on plain tensors, bit for bit (ECHOBlock's dense tail: 1e-5), and they run
through the C++ nodes and through the Python nodes."""
import numpy as np
import pytest
import torch

import _dynamic_range_cases as drc
import _lift_echo_cases as lc
import _losses_ref
import _matching_ref
import _pointwise_cases as pc
import _wide_runtime_cases as wrc          # noqa: F401  (registers its shapes with _dynamic_range_cases)
from conftest import load_golden, rel_err
from oracle import fieldconv_oracle as orc
from test_gpu_dynamic_range import TOL as CONV_TOL, build_graph
from test_gpu_losses import F32_GATE
from test_gpu_mesh_batch import TOL as POOL_TOL, pool_ref
from test_gpu_pointwise import TOL as POINT_TOL, TOL_F64
from test_gpu_wide_runtime import RT_GATES, WIDE_GATES, build_graph as build_wide_graph
from test_tensor_contract_host import dense_neg, every_other, expanded_row, forms_of, lazy_conj, lazy_neg, offset_view, transposed

pytestmark = pytest.mark.gpu
FORMS = {'lazy_conj': lazy_conj, 'lazy_neg': lazy_neg, 'dense_neg': dense_neg, 'transposed': transposed, 'every_other': every_other,
         'offset': offset_view, 'expanded': expanded_row}
CONV_GATES = (CONV_TOL, 5 * CONV_TOL, CONV_TOL)


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'GPU tests need a ROCm device'
    return torch.device('cuda:0')


def H(t):
    return t.detach().resolve_conj().resolve_neg().cpu().numpy()


def D(a, dev):
    return torch.from_numpy(np.array(a)).to(dev)


class _Ref(dict):
    """a reference {output: array} that carries `own`, the errors of the float32 restatement on the same arguments: the gates of the
    TransField and ECHO tests are multiples of them (lc.gate_of)"""


class Row:
    """args: numpy inputs; cot: numpy cotangent (None: the operator is not differentiable); op(*device tensors) -> output or tuple of
    outputs; ref(args, cot) -> tuple of references (outputs, then one gradient per argument outside `nograd`); errs(got, ref) ->
    [(label, error, gate)], an error of 0 with gate 0 meaning bit-equal (<=)"""

    def __init__(self, args, cot, op, ref, errs, nograd=()):
        self.args, self.cot, self.op, self.ref, self.errs, self.nograd = args, cot, op, ref, errs, set(nograd)


# ------------------------------------------------------------------------------------------------------------- FieldConv rows
def _conv_errs(name, gates):
    def errs(got, ref):
        e = drc.errors(name, 'random', (got[0], got[1], got[2]), (ref[0], ref[1], ref[2]))
        return [(label, v, g) for label, v, g in zip(('y', 'gx', 'gW'), e, gates)]
    return errs


def _row_field_conv(dev, name, build=build_graph, gates=CONV_GATES):
    from fieldconv_amd.functional import field_conv
    graph = build(name, dev)
    edges, sten = drc.mesh(name)[:2]
    x, gy, W = drc.scaled_inputs(name, 'random', 0, 0)

    def ref(args, cot):
        return orc.fieldconv_forward_backward(args[0].astype(np.complex128), edges, sten.astype(np.complex128), args[1].astype(np.complex128),
                                              cot.astype(np.complex128))
    return Row([x, W], gy, lambda x, w: field_conv(x, w, graph), ref, _conv_errs(name, gates))


def _row_field_conv_params(dev, name, ftype, build=build_graph, gates=CONV_GATES, act=False):
    """the parameter path; act: modReLU(conv(x) + addend) in the convolution's epilogue (field_conv_act)"""
    from fieldconv_amd.functional import field_conv_act, field_conv_params
    N, k, I, O, B, R = drc.dims(name)
    graph = build(name, dev)
    edges, sten = drc.mesh(name)[:2]
    x, gy, _ = drc.scaled_inputs(name, 'random', 0, 0)
    z, s, p = drc.scaled_params(name, 'random', ftype)
    n_par = 3 if ftype == 1 else 2
    args = [x, z, s] + ([p] if ftype == 1 else [])
    rng = np.random.default_rng(O)
    if act:
        bias = rng.uniform(-0.4, 0.1, O).astype(np.float32)
        addend = (0.25 * (rng.standard_normal((N, O)) + 1j * rng.standard_normal((N, O)))).astype(np.complex64)
        args += [bias, addend]
    pdev = D(p, dev)

    def op(x, z, s, *rest):
        rest = list(rest)
        ph = rest.pop(0) if ftype == 1 else pdev
        if act:
            return field_conv_act(x, z, s, ph, ftype, B, graph, rest[0], rest[1])
        return field_conv_params(x, z, s, ph, ftype, B, graph)

    def ref(args, cot):
        zz, ss = args[1].astype(np.float64), args[2].astype(np.float64)
        pp = (args[3] if ftype == 1 else p).astype(np.float64)
        W = orc.effective_filter(zz, ss, pp, ftype, B)
        xx, st, g = args[0].astype(np.complex128), sten.astype(np.complex128), cot.astype(np.complex128)
        tail = ()
        if act:
            bb, add = args[-2].astype(np.float64).reshape(1, -1), args[-1].astype(np.complex128)
            pre = orc.fieldconv_forward_backward(xx, edges, st, W, g)[0] + add
            y = orc.tangent_nonlin_forward(pre, bb)
            g, gb = orc.tangent_nonlin_backward(pre, bb, g)
            tail = (np.asarray(gb).reshape(-1), g)
            gx, gW = orc.fieldconv_forward_backward(xx, edges, st, W, g)[1:]
        else:
            y, gx, gW = orc.fieldconv_forward_backward(xx, edges, st, W, g)
        pref = orc.effective_filter_vjp(gW, zz, ss, pp, ftype, B)
        return (y, gx) + tuple(pref[:n_par]) + tail

    def errs(got, ref):
        ey, egx, _ = drc.errors(name, 'random', (got[0], got[1], ref[1]), (ref[0], ref[1], ref[1]))
        out = [('y', ey, gates[0]), ('gx', egx, gates[1])]
        out += [('g_' + n, drc.measured_err(g, r), gates[2]) for n, g, r in zip(('zonal', 'spherical', 'phase')[:n_par], got[2:], ref[2:])]
        if act:
            out += [('g_bias', rel_err(got[-2].reshape(-1), ref[-2]), gates[2]), ('g_addend', drc.measured_err(got[-1], ref[-1]), gates[1])]
        return out
    return Row(args, gy, op, ref, errs)


# ------------------------------------------------------------------------------------------------------------- pointwise rows
def _row_tangent_lin(dev, which):
    from fieldconv_amd.functional import tangent_lin
    case = pc.lin_cases(torch.cuda.get_device_properties(dev).multi_processor_count)[which]
    assert case.offset == 0
    x, gy, Re, Im, _ = pc.inputs(case.N, case.I, case.O)

    def ref(args, cot):
        a = (args[0].astype(np.complex128), args[1].astype(np.float64), args[2].astype(np.float64))
        return (orc.tangent_lin_forward(*a),) + tuple(orc.tangent_lin_backward(*a, cot.astype(np.complex128)))

    def errs(got, ref):
        return [('y', pc.rowwise_err(got[0], ref[0]), POINT_TOL), ('gx', pc.rowwise_err(got[1], ref[1]), POINT_TOL),
                ('gRe', rel_err(got[2], ref[2]), POINT_TOL), ('gIm', rel_err(got[3], ref[3]), POINT_TOL)]
    return Row([x, Re, Im], gy, tangent_lin, ref, errs)


def _row_tangent_nonlin(dev, N, C, f64=False):
    """f64: the double-precision kernels on the complex128 values of the same inputs; numpy's complex128 restatement is good to a few
    ulp (1e-15), three orders inside the gate of the kernels' own test (1e-12, there against longdouble)"""
    from fieldconv_amd.functional import tangent_nonlin
    x, gy, _, _, bias = pc.inputs(N, C, C)
    gate = TOL_F64 if f64 else POINT_TOL
    if f64:
        x, gy, bias = x.astype(np.complex128), gy.astype(np.complex128), bias.astype(np.float64)

    def ref(args, cot):
        xx, bb = args[0].astype(np.complex128), args[1].astype(np.float64)
        gx, gb = orc.tangent_nonlin_backward(xx, bb, cot.astype(np.complex128))
        return orc.tangent_nonlin_forward(xx, bb), gx, np.asarray(gb)

    def errs(got, ref):
        return [('y', pc.rowwise_err(got[0], ref[0]), gate), ('gx', pc.rowwise_err(got[1], ref[1]), gate),
                ('gbias', rel_err(got[2].reshape(-1), ref[2].reshape(-1)), gate)]
    return Row([x, bias], gy, tangent_nonlin, ref, errs)


def _row_soft_abs(dev, N, C):
    from fieldconv_amd.functional import soft_abs
    x, gy = pc.inputs(N, C, C)[:2]

    def ref(args, cot):          # (_pointwise_cases.soft_abs_reference, on the arguments at hand)
        xx, g = args[0].astype(np.complex128), cot.astype(np.float64)
        box = pc.origin_box(xx)
        r = np.where(box, 1.0, np.abs(xx))
        return np.where(box, 0.0, np.abs(xx)), np.where(box, 0.0, g * xx / r)

    def errs(got, ref):
        return [('y', pc.rowwise_err(got[0], ref[0]), POINT_TOL), ('gx', pc.rowwise_err(got[1], ref[1]), POINT_TOL)]
    return Row([x], np.ascontiguousarray(gy.real), soft_abs, ref, errs)


# ------------------------------------------------------------------------------------------------------- TransField and ECHO rows
def _row_trans_field(dev, name):
    from fieldconv_amd import functional as Fn
    m, Cin, R, O, ftype, layout, f64 = lc.tf_case(name)
    assert ftype == 1 and not f64
    p = lc.tf_problem(name)
    edges = D(p['edges'], dev)

    def op(x, sten, za, zm, ph):
        assert Fn.trans_field_specialised(x, sten, za) == lc.tf_specialised(Cin, R, O, f64)
        return Fn.trans_field(x, edges, sten, za, zm, ph, ftype)

    def ref(args, cot):
        q = dict(p, s01=args[1], zonalAng=args[2], zonalMag=args[3], phase=args[4])
        want = _Ref(lc._tf_run(q, torch.float64, ftype, x=args[0], gy=cot))          # {y, gx, g_zonalAng, g_zonalMag, g_phase}
        want.own = lc.tf_errors(lc._tf_run(q, torch.float32, ftype, x=args[0], gy=cot), want)
        return want

    def errs(got, ref):
        e = lc.tf_errors(dict(zip(lc.TF_OUTPUTS, got)), ref)
        return [(k, e[k], lc.gate_of(ref.own[k])) for k in lc.TF_OUTPUTS if k in e]
    return Row([p['x'], p['s01'], p['zonalAng'], p['zonalMag'], p['phase']], p['gy'], op, ref, errs, nograd=(1,))


def _row_echo(dev, name):
    from fieldconv_amd.nn import ECHO
    m, C, n_bins, layout, c128 = lc.echo_case(name)
    assert not c128
    p = lc.echo_problem(name)
    edges, ln, wxp = D(p['edges'], dev), D(p['ln'], dev), D(p['wxp'], dev)
    mod = ECHO(C, n_bins).to(dev)

    def ref(args, cot):
        want = _Ref(lc._echo_run(p, n_bins, torch.complex128, x=args[0], gd=cot))
        want.own = lc.echo_errors(name, lc._echo_run(p, n_bins, torch.complex64, x=args[0], gd=cot), want)
        return want

    def errs(got, ref):          # (the masks are those of the case's own x: every form has its value)
        e = lc.echo_errors(name, dict(desc=got[0], gx=got[1]), ref)
        return [('desc', e[0], lc.gate_of(ref.own[0])), ('gx', e[1], lc.gate_of(ref.own[1]))]
    return Row([p['x']], p['gd'], lambda x: mod(x, edges, ln, wxp), ref, errs)


# --------------------------------------------------------------------------------------------------- pooling, losses, matching
def _row_mesh_pool(dev, C, soft_abs, reduce):
    """three meshes, the middle one empty"""
    from fieldconv_amd.pooling import mesh_pool
    rng = np.random.default_rng(C)
    sizes = (70, 0, 9)
    N = sum(sizes)
    ptr = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    if soft_abs:
        x = (rng.standard_normal((N, C)) + 1j * rng.standard_normal((N, C))).astype(np.complex64)
        x[3, 0], x[7, :] = 0, 0
        x[71, C - 1] = complex(5e-8, -5e-8)              # inside the origin box
    else:
        x = rng.standard_normal((N, C)).astype(np.float32)
    g = rng.standard_normal((3, C)).astype(np.float32)
    ptr_d = D(ptr, dev)

    def ref(args, cot):
        return pool_ref(args[0], ptr, reduce, soft_abs, cot.astype(np.float64))

    def errs(got, ref):
        return [('out', rel_err(got[0], ref[0]), POOL_TOL), ('gx', rel_err(got[1], ref[1]), POOL_TOL)]
    return Row([x], g, lambda x: mesh_pool(x, ptr_d, reduce, soft_abs), ref, errs)


def _row_twin_loss(dev):
    from fieldconv_amd.losses import twin_loss
    c = load_golden('losses.npz')['twin_n300']
    p_, n_, mu = D(c['p'], dev), D(c['n'], dev), float(c['mu'])
    xS, xT, yN = c['xS'].astype(np.float32), c['xT'].astype(np.float32), c['yN'].astype(np.float32)

    def ref(args, cot):
        lp, ln, gS, gT = _losses_ref.twin_loss(args[0], args[1], c['p'], c['n'], args[2], mu)
        g = float(np.asarray(cot, np.float64).reshape(-1)[0])
        return np.array([lp + ln]), g * gS, g * gT

    def errs(got, ref):
        return [('loss', rel_err(got[0].astype(np.float64), ref[0]), F32_GATE), ('gS', rel_err(got[1], ref[1]), F32_GATE),
                ('gT', rel_err(got[2], ref[2]), F32_GATE)]
    return Row([xS, xT, yN], np.array([0.75], np.float32), lambda s, t, y: twin_loss(s, t, p_, n_, y, mu), ref, errs, nograd=(2,))


def _row_pair_sqdist(dev):
    """bit for bit the numpy restatement, as in test_pair_sqdist_is_bit_exact (its smallest shape with more than one tile)"""
    from fieldconv_amd.losses import pair_sqdist
    rng = np.random.default_rng(65 + 17)
    n_T, n_S, C = 65, 63, 17
    xS, xT = (0.9 * rng.random((n_S, C))).astype(np.float32), (0.9 * rng.random((n_T, C))).astype(np.float32)
    pairs = np.stack((rng.integers(0, n_T, 500), rng.integers(0, n_S, 500)), 1)
    pd = D(pairs, dev)

    def ref(args, cot):
        return (_losses_ref.sqdist(args[1][pairs[:, 0]], args[0][pairs[:, 1]]),)

    def errs(got, ref):
        return [('d2 bits', float(not np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))), 0.0)]
    return Row([xS, xT], None, lambda s, t: pair_sqdist(s, t, pd), ref, errs)


def _row_match(dev):
    """idx and the distance bits equal the restatement, as in test_matches_equal_the_restatement"""
    from fieldconv_amd.matching import match_descriptors
    rng = np.random.default_rng(17)
    n_T, n_S, C, k = 65, 63, 17, 3
    xS, xT = rng.standard_normal((n_S, C)).astype(np.float32), rng.standard_normal((n_T, C)).astype(np.float32)

    def ref(args, cot):
        return _matching_ref.topk(args[0], args[1], k)

    def errs(got, ref):
        return [('idx', float(not np.array_equal(got[0], ref[0])), 0.0),
                ('d2 bits', float(not np.array_equal(got[1].view(np.uint32), ref[1].view(np.uint32))), 0.0)]
    return Row([xS, xT], None, lambda s, t: match_descriptors(s, t, k), ref, errs)


def _row_label_smoothing(dev, shape):
    from fieldconv_amd.losses import label_smoothing_loss
    c = load_golden('losses.npz')[shape]
    pred, weight, target = c['pred'].astype(np.float32), c['weight'].astype(np.float32), c['target']
    K = pred.shape[1]
    td = D(target, dev)

    def ref(args, cot):
        loss, grad = _losses_ref.label_smoothing(args[0], target, K, 0.1, args[1])
        return np.array(loss), float(np.asarray(cot, np.float64).reshape(-1)[0]) * grad

    def errs(got, ref):
        return [('loss', rel_err(got[0].astype(np.float64), ref[0]), F32_GATE), ('gpred', rel_err(got[1], ref[1]), F32_GATE)]
    return Row([pred, weight], np.array(0.75, np.float32), lambda p, w: label_smoothing_loss(p, td, K, 0.1, w), ref, errs, nograd=(1,))


ROWS = {
    'field_conv-split60': lambda dev: _row_field_conv(dev, drc.SMALLEST),
    'field_conv_params-param400-ftype0': lambda dev: _row_field_conv_params(dev, 'param400', 0),
    'field_conv_params-param400-ftype1': lambda dev: _row_field_conv_params(dev, 'param400', 1),
    'field_conv_params-param400-ftype2': lambda dev: _row_field_conv_params(dev, 'param400', 2),
    'field_conv_act-param400': lambda dev: _row_field_conv_params(dev, 'param400', 1, act=True),
    'field_conv-wide129': lambda dev: _row_field_conv(dev, 'wide129', build_wide_graph, WIDE_GATES),
    'field_conv_params-wide129': lambda dev: _row_field_conv_params(dev, 'wide129', 1, build_wide_graph, WIDE_GATES),
    'field_conv-rt_rings9': lambda dev: _row_field_conv(dev, 'rt_rings9', build_wide_graph, RT_GATES[torch.complex64]),
    'field_conv_params-rt_rings9': lambda dev: _row_field_conv_params(dev, 'rt_rings9', 1, build_wide_graph, RT_GATES[torch.complex64]),
    'tangent_lin-split-trip2': lambda dev: _row_tangent_lin(dev, 'split-trip2'),
    'tangent_lin-direct-k64': lambda dev: _row_tangent_lin(dev, 'direct-k64'),
    'tangent_nonlin-7-1': lambda dev: _row_tangent_nonlin(dev, 7, 1),
    'tangent_nonlin-5-130': lambda dev: _row_tangent_nonlin(dev, 5, 130),
    'tangent_nonlin-f64-7-1': lambda dev: _row_tangent_nonlin(dev, 7, 1, f64=True),
    'tangent_nonlin-f64-5-130': lambda dev: _row_tangent_nonlin(dev, 5, 130, f64=True),
    'soft_abs-7-1': lambda dev: _row_soft_abs(dev, 7, 1),
    'soft_abs-5-130': lambda dev: _row_soft_abs(dev, 5, 130),
    'trans_field-specialised': lambda dev: _row_trans_field(dev, 'size-%d-%d-%d-t1' % lc.TF_SPECIALISED_SIZES[1]),
    'trans_field-generic': lambda dev: _row_trans_field(dev, 'size-%d-%d-%d-t1' % lc.TF_GENERIC_SIZES[0]),
    'echo-rows-n42': lambda dev: _row_echo(dev, 'rows-n42'),          # (the smallest mesh with more than one vertex)
    'mesh_pool-softabs-mean-3': lambda dev: _row_mesh_pool(dev, 3, True, 'mean'),
    'mesh_pool-softabs-sum-130': lambda dev: _row_mesh_pool(dev, 130, True, 'sum'),
    'mesh_pool-real-mean-130': lambda dev: _row_mesh_pool(dev, 130, False, 'mean'),
    'mesh_pool-real-sum-3': lambda dev: _row_mesh_pool(dev, 3, False, 'sum'),
    'twin_loss': _row_twin_loss,
    'pair_sqdist': _row_pair_sqdist,
    'label_smoothing-ls_1x30': lambda dev: _row_label_smoothing(dev, 'ls_1x30'),
    'label_smoothing-ls_257x40': lambda dev: _row_label_smoothing(dev, 'ls_257x40'),
    'match_descriptors': _row_match,
}


def test_the_rows_are_cases_of_the_case_lists():
    assert {'split-trip2', 'direct-k64'} <= set(pc.LIN_NAMES) and (7, 1) in pc.NONLIN_SHAPES and (5, 130) in pc.NONLIN_SHAPES
    assert 'wide129' in wrc.WIDE_SHAPES and 'rt_rings9' in wrc.RT_SHAPES and 'rows-n42' in lc.ECHO_CASES
    assert 'size-%d-%d-%d-t1' % lc.TF_SPECIALISED_SIZES[1] in lc.TF_CASES and 'size-%d-%d-%d-t1' % lc.TF_GENERIC_SIZES[0] in lc.TF_CASES


# ------------------------------------------------------------------------------------------------------------------------ the test
def _feed(row, dev, slot=None, form=None):
    """[(what the operator is given, the leaf gradients are asked of)]: the leaf itself, or at `slot` a form of it"""
    pairs = []
    for i, a in enumerate(row.args):
        leaf = D(a, dev)
        if row.cot is not None and i not in row.nograd:
            leaf.requires_grad_(True)
        pairs.append((form(leaf) if i == slot else leaf, leaf))
    return pairs


def _run(row, pairs, cot, through_conj=False):
    """(outputs..., gradients...) on the device"""
    y = row.op(*[fed for fed, _ in pairs])
    if row.cot is None:
        return tuple(t.detach() for t in (y if isinstance(y, tuple) else (y,)))
    roots = [leaf for i, (_, leaf) in enumerate(pairs) if i not in row.nograd]
    grads = torch.autograd.grad(y.conj() if through_conj else y, roots, grad_outputs=cot)
    return (y.detach(),) + tuple(grads)


def _check(name, row, got, ref, where):
    errs = row.errs([H(t) for t in got], ref)
    print('  %s: %s' % (where, ' '.join('%s %.2e' % (label, e) for label, e, _ in errs)))
    for label, e, gate in errs:
        assert e <= gate if gate == 0 else e < gate, (name, where, label, e, gate)


@pytest.mark.parametrize('name', sorted(ROWS))
def test_operator_computes_on_the_value_of_every_form(name, dev):
    row = ROWS[name](dev)
    diff = row.cot is not None
    cot_plain = D(row.cot, dev) if diff else None
    plain = _run(row, _feed(row, dev), cot_plain)
    again = _run(row, _feed(row, dev), cot_plain)
    assert all(torch.equal(a, b) for a, b in zip(plain, again)), 'two runs of the plain form differ in their bits'
    ref_plain = row.ref(row.args, row.cot)
    _check(name, row, plain, ref_plain, 'plain')

    # the condition on the inputs: conjugating a complex argument (or the cotangent) moves the reference by more than 100 gates
    slots = list(range(len(row.args))) + (['cot'] if diff else [])
    for slot in slots:
        a = row.cot if slot == 'cot' else row.args[slot]
        if not np.iscomplexobj(a):
            continue
        args = [np.conj(t) if i == slot else t for i, t in enumerate(row.args)]
        moved_ref = row.ref(args, np.conj(row.cot) if slot == 'cot' else row.cot)
        moved_ref = list(moved_ref.values()) if isinstance(moved_ref, dict) else list(moved_ref)
        moved = row.errs(moved_ref, ref_plain)
        assert max(e / gate for _, e, gate in moved) > 100, (name, slot, moved)

    for slot in slots:
        a = row.cot if slot == 'cot' else row.args[slot]
        for fname in forms_of(torch.from_numpy(np.array(a)), cotangent=slot == 'cot'):
            form = FORMS[fname]
            if slot == 'cot':
                cot, pairs = form(cot_plain), _feed(row, dev)
                odd = cot
            else:
                cot, pairs = cot_plain, _feed(row, dev, slot, form)
                odd = pairs[slot][0]
                assert np.array_equal(H(odd), a), (name, slot, fname)
            assert odd.is_conj() or odd.is_neg() or not odd.is_contiguous() or odd.storage_offset(), (name, slot, fname)
            got = _run(row, pairs, cot)
            if fname == 'expanded':          # another value: its own reference, and its own plain run
                ref, base = row.ref(row.args, H(cot)), _run(row, _feed(row, dev), cot.contiguous())
            else:
                assert not diff or np.array_equal(H(cot), row.cot)
                ref, base = ref_plain, plain
            _check(name, row, got, ref, '%s %s' % (slot, fname))
            for i, (g, b) in enumerate(zip(got, base)):
                assert torch.equal(g, b), (name, slot, fname, 'output %d differs from the plain form in its bits' % i)

    # the cotangent's bit from the graph itself: the only consumer of the output is .conj(); d/dx of <g, conj(y)> is the VJP of conj(g)
    if diff and plain[0].is_complex():
        got = _run(row, _feed(row, dev), cot_plain, through_conj=True)
        ref = row.ref(row.args, np.conj(row.cot))
        base = _run(row, _feed(row, dev), cot_plain.conj().resolve_conj())
        _check(name, row, got, ref, 'conj in the graph')
        for i, (g, b) in enumerate(zip(got[1:], base[1:])):
            assert torch.equal(g, b), (name, 'conj in the graph', i)


# ----------------------------------------------------------------------------------------------- the block-level entry points
BLOCKS = [('resnet', None), ('lift', None), ('echo', None), ('echo', 'aten')]          # (module, FIELDCONV_ECHO_TAIL)


@pytest.fixture(scope='module')
def block_mesh(dev):
    """N = 77, k = 9 and the channel counts of test_block_level_entry_points_match_the_per_operator_path's first case"""
    from fieldconv_amd.data import sphere_support
    from fieldconv_amd.transforms import FCPrecomp
    N, k, cin, cout, B, R = 77, 9, 16, 24, 2, 6
    data = sphere_support(N, k, seed=N).to(dev)
    edges, sten, ln, wxp = FCPrecomp(B, R, data.epsilon)(data)
    g = torch.Generator().manual_seed(N)
    x = torch.complex(torch.randn(N, cin, generator=g), torch.randn(N, cin, generator=g))
    x[torch.rand(N, cin, generator=g) < 0.02] = 0
    return dict(N=N, cin=cin, cout=cout, B=B, R=R, edges=edges, sten=sten, ln=ln, wxp=wxp, x=x, pos=torch.randn(N, 3, generator=g))


def _block(which, m, dev):
    from fieldconv_amd.nn import ECHOBlock, FCResNetBlock, LiftBlock
    torch.manual_seed(m['N'])
    if which == 'resnet':
        mod = FCResNetBlock(m['cin'], m['cout'], band_limit=m['B'], n_rings=m['R']).to(dev)
        biases, inp, rest = (mod.nonlin1.bias, mod.nonlin2.bias), m['x'], (m['edges'], m['sten'])
    elif which == 'echo':
        mod = ECHOBlock(m['cin'], 7, n_des=m['cin'], n_bins=3, band_limit=m['B'], n_rings=m['R']).to(dev)
        biases, inp, rest = (mod.nonlin.bias,), m['x'], (m['edges'], m['sten'], m['ln'], m['wxp'])
    else:
        mod = LiftBlock(3, m['cout'], n_rings=m['R'], ftype=1).to(dev)
        biases, inp, rest = (mod.nonlin.bias,), m['pos'], (m['edges'], m['sten'][..., m['B']:m['B'] + 2])
    with torch.no_grad():
        for b in biases:
            b.uniform_(-0.4, 0.1)
    return mod, inp.to(dev), rest


def _owners(mod):
    """[(module, name, parameter)] of every parameter"""
    return [(sub, n, p) for sub in mod.modules() for n, p in list(sub._parameters.items()) if p is not None]


def _block_run(mod, x, rest, cot, slot=None, form=None, through_conj=False):
    """(y, gx, every parameter gradient): `slot` 'x' or the index of a parameter, fed as form(leaf) -- a parameter by standing in for it
    in its module's table -- with the gradients asked of the leaves"""
    owners = _owners(mod)
    xl = x.detach().clone().requires_grad_(True)
    if isinstance(slot, int):
        sub, n, p = owners[slot]
        sub._parameters[n] = form(p)
    try:
        y = mod(form(xl) if slot == 'x' else xl, *rest)
        grads = torch.autograd.grad(y.conj() if through_conj else y, [xl] + [p for _, _, p in owners], grad_outputs=cot, allow_unused=True)
    finally:
        if isinstance(slot, int):
            sub._parameters[n] = p
    return (y.detach(),) + tuple(grads)


def _node_in(y, names):
    seen, todo, found = set(), [y.grad_fn], set()
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        found |= {(n, 'cpp' if 'CppNode' in fn.name() else 'python') for n in names if n in fn.name()}
        todo += [nf for nf, _ in fn.next_functions]
    return found


@pytest.mark.parametrize('route', ['cpp', 'python'])
@pytest.mark.parametrize('which,tail', BLOCKS, ids=['resnet', 'lift', 'echo-head', 'echo-tail'])
def test_block_level_nodes_compute_on_the_value_of_every_form(which, tail, route, dev, block_mesh, monkeypatch):
    from fieldconv_amd.blocks import cpp_nodes
    assert cpp_nodes() is not None, 'fc_torch_nodes.so (the C++ autograd nodes) is not built'
    m = block_mesh
    mod, x, rest = _block(which, m, dev)
    with torch.no_grad():
        y0 = mod(x, *rest)
    gen = torch.Generator().manual_seed(1)
    cot = torch.randn(y0.shape, generator=gen)
    if y0.is_complex():
        cot = torch.complex(cot, torch.randn(y0.shape, generator=gen))
    cot = cot.to(dev)
    gate = 1e-5 if which == 'echo' else 0.0          # (the dense tail against torch's Linear nodes: test_block_level_entry_points_...)

    def reference(xv, cv):
        """the per-operator composition on plain tensors"""
        monkeypatch.setenv('FIELDCONV_BLOCK_CALLS', '0')
        monkeypatch.setenv('FIELDCONV_CPP_NODES', '0')
        monkeypatch.setenv('FIELDCONV_ECHO_TAIL', '0')
        return _block_run(mod, xv, rest, cv)

    def block_route():
        monkeypatch.setenv('FIELDCONV_BLOCK_CALLS', '1')
        monkeypatch.setenv('FIELDCONV_CPP_NODES', '1' if route == 'cpp' else '0')
        if tail is None:
            monkeypatch.delenv('FIELDCONV_ECHO_TAIL', raising=False)
        else:
            monkeypatch.setenv('FIELDCONV_ECHO_TAIL', tail)

    def against(got, ref, where):
        for i, (a, b) in enumerate(zip(got, ref)):
            assert (a is None) == (b is None), (where, i)
            if a is None:
                continue
            if gate:
                e = rel_err(H(a), H(b))
                assert e < gate, (which, route, where, i, e)
            else:
                assert torch.equal(a, b), (which, route, where, i)

    ref_plain = reference(x, cot)
    if x.is_complex():          # the condition on the inputs, on the reference alone
        moved = reference(x.conj().resolve_conj(), cot)          # (ECHO's descriptors barely see a reflection: the gradients do)
        assert max(rel_err(H(a), H(b)) for a, b in zip(moved, ref_plain) if a is not None) > 100 * max(gate, 1e-5)
    if cot.is_complex():
        moved = reference(x, cot.conj().resolve_conj())
        assert rel_err(H(moved[1]), H(ref_plain[1])) > 100 * max(gate, 1e-5)

    block_route()
    xl = x.detach().clone().requires_grad_(True)
    nodes = {'resnet': ['ResnetBlockFn'], 'lift': ['LiftBlockFn'], 'echo': ['EchoBlockFn', 'EchoTailFn' if tail else 'EchoHeadFn']}[which]
    assert _node_in(mod(xl, *rest), nodes) == {(n, route) for n in nodes}
    plain = _block_run(mod, x, rest, cot)
    again = _block_run(mod, x, rest, cot)
    assert all((a is None and b is None) or torch.equal(a, b) for a, b in zip(plain, again)), 'two plain runs differ in their bits'
    against(plain, ref_plain, 'plain')

    owners = _owners(mod)
    slots = ['x'] + list(range(len(owners))) + ['cot']
    for slot in slots:
        t = x if slot == 'x' else cot if slot == 'cot' else owners[slot][2].detach()
        for fname in forms_of(t, cotangent=slot == 'cot'):
            form = FORMS[fname]
            where = '%s %s' % (slot if not isinstance(slot, int) else owners[slot][1] + '#%d' % slot, fname)
            if slot == 'cot':
                fed = form(cot)
                got = _block_run(mod, x, rest, fed)
            else:
                fed = form(t)
                got = _block_run(mod, x, rest, cot, slot, form)
            assert fed.is_conj() or fed.is_neg() or not fed.is_contiguous() or fed.storage_offset(), where
            if fname == 'expanded':
                plain_value = fed.contiguous()
                base = _block_run(mod, x, rest, plain_value)
                ref = reference(x, plain_value)
                block_route()
            else:
                assert torch.equal(fed, t), where
                base, ref = plain, ref_plain
            against(got, ref, where)
            for i, (a, b) in enumerate(zip(got, base)):
                assert (a is None and b is None) or torch.equal(a, b), (which, route, where, 'output %d differs from the plain form in its bits' % i)

    if y0.is_complex():          # the cotangent's bit from the graph itself
        got = _block_run(mod, x, rest, cot, through_conj=True)
        base = _block_run(mod, x, rest, cot.conj().resolve_conj())
        for i, (a, b) in enumerate(zip(got[1:], base[1:])):
            assert (a is None and b is None) or torch.equal(a, b), (which, route, 'conj in the graph', i)
