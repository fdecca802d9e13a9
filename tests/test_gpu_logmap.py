"""The device's log map and transport (fieldconv_amd.logmap, csrc/fc_logmap.hip) against the numpy restatement
tests/_logmap_ref.py.  Frames and trees are compared exactly: they are float32 operations in a fixed order, and integer and bit
decisions on a field that has the same bits everywhere.  Values are compared with the float64 restatement on the same tree; the
gate is not fixed in advance but measured per case: 4 x the float32 restatement's own error against float64, with a floor of
1e-6 of the largest |L| (the scheme of tests/test_gpu_head.py).  Angles are only ever compared as unit complex numbers."""
import functools

import numpy as np
import pytest
import torch

import _geodesic_ref as gref
import _logmap_ref as lref
from _logmap_ref import ICO_BOUND, closed_form, closed_form_errors, ico_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def bits(t):
    return torch.view_as_real(t).view(torch.int32) if t.is_complex() else (t.view(torch.int32) if t.dtype == torch.float32 else t)


# eight samples of the strip above the LDS capacity of the relaxation state, some within reach of each other
CLUSTERED = np.array([0, 4, 9, 3000, 3003, 10000, 10001, 20000], dtype=np.int64)
TWO_SAMPLES = np.array([0, 7, 14, 20, 29, 33, 40, 45, 46, 47], dtype=np.int64)


# every reference is computed once and shared (the tests only read it)
@functools.lru_cache(maxsize=None)
def case(name):
    if name == 'ico':
        return ico_case()
    if name == 'grid':
        pos, face = lref.jittered_grid(9, 9)
        return lref.Case(pos, face, np.arange(81), lref.all_pairs(81), 0.6)
    if name == 'two':
        pos, face = lref.two_components()
        return lref.Case(pos, face, TWO_SAMPLES, lref.all_pairs(len(TWO_SAMPLES)), 0.4)
    if name == 'strip':          # 20 001 vertices: the relaxation state in global memory
        pos, face = gref.lattice(6667, 3)
        return lref.Case(pos, face, CLUSTERED, lref.all_pairs(len(CLUSTERED)), 0.375)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def device_result(name, ball_lds=None, tree=False):
    from fieldconv_amd.logmap import log_map_transport
    c, dev = case(name), torch.device('cuda:0')
    return log_map_transport(T(c.pos, dev), T(c.face, dev), T(c.sample_idx, dev), T(c.edges, dev), c.bound, return_reached=True,
                             return_tree=tree, ball_lds_vertices=ball_lds)


def rebuilt(mag, ang):
    """L as a complex number from the polar pair, in float64"""
    return mag.astype(np.float64) * np.exp(1j * ang.astype(np.float64))


@functools.lru_cache(maxsize=None)
def gates(name):
    """(L64, X64 complex, gate of L, gate of X, the float32 restatement's errors)"""
    c = case(name)
    (L32, X32), (L64, X64) = c.values(np.float32), c.values(np.float64)
    L64c, X64c = lref.as_complex(L64), lref.as_complex(X64)
    own_L = float(np.abs(rebuilt(*lref.polar(L32)) - L64c).max())          # through the polar pair, as the device's rows are
    own_X = float(np.abs(lref.as_complex(X32) - X64c).max())
    top = float(np.abs(L64c).max())
    return L64c, X64c, max(4 * own_L, 1e-6 * top), max(4 * own_X, 1e-6), own_L, own_X


def device_values(name):
    mag, ang, xp, reached = device_result(name)[:4]
    return rebuilt(N_(mag), N_(ang)), N_(xp).astype(np.complex128), N_(reached)


# ------------------------------------------------------------------ 1. frames
@pytest.mark.parametrize('mesh', ['ico', 'odd'])
def test_frames_equal_the_float32_restatement(dev, mesh):
    from fieldconv_amd.logmap import vertex_frames
    pos, face = lref.icosphere(3) if mesh == 'ico' else lref.frames_mesh()
    assert pos.shape[0] == (642 if mesh == 'ico' else 62)
    want = lref.frames(pos, face, np.float32)
    if mesh == 'odd':
        assert np.array_equal(want[0][60], [0, 0, 1]) and np.isfinite(want[0]).all()          # the isolated vertex
    got = vertex_frames(T(pos, dev), T(face, dev))
    for g, w in zip(got, want):
        assert g.device == dev and g.dtype == torch.float32
        assert np.array_equal(N_(g).view(np.uint32), w.view(np.uint32))


# ------------------------------------------------------------------ 2. tree
@pytest.mark.parametrize('name', ['ico', 'grid', 'two', 'strip'])
def test_tree_equals_the_restatement(dev, name):
    c = case(name)
    pred, hops = device_result(name, tree=True)[4:6]
    assert pred.dtype == torch.int32 and tuple(pred.shape) == c.pred.shape
    assert np.array_equal(N_(hops), c.h)
    assert np.array_equal(N_(pred), c.pred)


# ------------------------------------------------------------------ 3. values
@pytest.mark.parametrize('name', ['ico', 'grid', 'two', 'strip'])
def test_values_against_float64_on_the_same_tree(dev, name):
    L64, X64, gate_L, gate_X, own_L, own_X = gates(name)
    L, X, reached = device_values(name)
    err_L, err_X = float(np.abs(L - L64).max()), float(np.abs(X - X64).max())
    print(f'\n{name}: device against float64 L {err_L:.3e} X {err_X:.3e}; float32 restatement against float64 L {own_L:.3e} '
          f'X {own_X:.3e}; gates {gate_L:.3e} {gate_X:.3e}')
    assert np.array_equal(reached, case(name).reached)
    assert err_L <= gate_L and err_X <= gate_X
    same = case(name).edges[:, 0] == case(name).edges[:, 1]          # a row [a, a] gives 0, 0, 1 exactly
    mag, ang, xp = device_result(name)[:3]
    assert bool((mag[T(same, dev)] == 0).all()) and bool((ang[T(same, dev)] == 0).all()) and bool((xp[T(same, dev)] == 1).all())


# ------------------------------------------------------------------ 4. closed form
def test_icosphere_against_the_closed_form(dev):
    """the device is as close to synthetic's closed-form sphere as the float64 restatement is, up to the gate of case 3: |dL| <=
    gate moves a magnitude by at most gate / dist relative and an angle by at most about gate / |L|; |dX| <= gate moves arg(xp)
    by about gate (asin(g) <= 1.01 g here)"""
    c = ico_case()
    L64, X64, gate_L, gate_X = gates('ico')[:4]
    L, X, _ = device_values('ico')
    as2 = lambda z: np.stack((z.real, z.imag), 1)
    ref = closed_form_errors(c, *c.values(np.float64))
    got = closed_form_errors(c, as2(L), as2(X))
    off = c.edges[:, 0] != c.edges[:, 1]
    shortest = float(min(closed_form(c)[0][off].min(), np.abs(L64[off]).min()))
    print(f'\nagainst the closed form (logMag relative, logAng rad, arg(xp) rad): device {got}, float64 restatement {ref}')
    assert got[0] <= ref[0] + gate_L / shortest
    assert got[1] <= ref[1] + 1.01 * gate_L / shortest
    assert got[2] <= ref[2] + 1.01 * gate_X


# ------------------------------------------------------------------ 5. planar grid
def test_planar_grid_xp_is_one_and_L_the_displacement(dev):
    c = case('grid')
    gate_L, gate_X = gates('grid')[2:4]
    L, X, _ = device_values('grid')
    _, e1, e2 = lref.frames(c.pos, c.face, np.float64)
    a = c.edges[:, 0]
    disp = c.pos[c.edges[:, 1]].astype(np.float64) - c.pos[a].astype(np.float64)
    want = (disp * e1[a]).sum(1) + 1j * (disp * e2[a]).sum(1)
    assert np.abs(X - 1).max() <= gate_X
    assert np.abs(L - want).max() <= gate_L


# ------------------------------------------------------------------ 6. fallback
def test_rows_not_reached_take_the_virtual_edge(dev):
    c = case('two')
    L64, X64, gate_L, gate_X = gates('two')[:4]
    L, X, reached = device_values('two')
    s, t = c.sample_idx[c.edges[:, 0]], c.sample_idx[c.edges[:, 1]]
    part = lambda v: np.where(v == 46, 2, np.where((v >= 30) & (v < 46), 1, 0))          # (47 is joined to 14; 46 is in no face)
    other = part(s) != part(t)                                                # the target lies in another component
    beyond = ~other & ~c.reached
    assert other.any() and beyond.any() and c.reached.sum() > len(TWO_SAMPLES)
    assert np.array_equal(reached, ~(other | beyond))
    out = ~reached
    assert np.isfinite(L[out]).all() and np.abs(L[out] - L64[out]).max() <= gate_L and np.abs(X[out] - X64[out]).max() <= gate_X
    chord = np.linalg.norm(c.pos[t].astype(np.float64) - c.pos[s].astype(np.float64), axis=1)
    assert np.abs(np.abs(L[out]) - chord[out]).max() <= gate_L                # the mesh is planar: the virtual edge keeps its length


def test_geodesic_support_graph_rows_are_all_reached(dev):
    from types import SimpleNamespace
    from fieldconv_amd.logmap import log_map_transport
    from fieldconv_amd.transforms import GeodesicSupportGraph
    c = ico_case()
    p, f = T(c.pos, dev), T(c.face, dev)
    data = GeodesicSupportGraph(epsilon=ICO_BOUND, sample_n=128, random_start=False)(SimpleNamespace(pos=p, face=f))
    assert np.array_equal(N_(data.sample_idx), c.sample_idx) and np.array_equal(N_(data.supp_edges), c.edges)
    reached = log_map_transport(p, f, data.sample_idx, data.supp_edges, ICO_BOUND, return_reached=True)[3]
    assert reached.dtype == torch.bool and bool(reached.all())


# ------------------------------------------------------------------ 7. memory paths, batching, row order
@pytest.mark.parametrize('name', ['ico', 'grid', 'two', 'strip'])
def test_lds_and_workspace_balls_give_the_same_bits(dev, name):
    """ball_lds_vertices = 0 sends every ball's tree state to the workspace slot; 'strip' relaxes in global memory either way, and
    a bound that takes in the whole 81-vertex grid with room for 32 vertices in LDS crosses the threshold inside one launch"""
    from fieldconv_amd.logmap import log_map_transport
    a, b = device_result(name, tree=True), device_result(name, ball_lds=0, tree=True)
    for x, y in zip(a, b):
        assert torch.equal(bits(x), bits(y))
    if name == 'grid':
        c = case(name)
        mixed = log_map_transport(T(c.pos, dev), T(c.face, dev), T(c.sample_idx, dev), T(c.edges, dev), c.bound, return_reached=True,
                                  return_tree=True, ball_lds_vertices=32)
        sizes = (c.h >= 0).sum(1)
        assert sizes.min() <= 32 < sizes.max()
        for x, y in zip(a, mixed):
            assert torch.equal(bits(x), bits(y))


def test_batch_equals_single_calls_and_rows_keep_their_order(dev):
    from fieldconv_amd.logmap import log_map_transport
    g, i = case('grid'), case('ico')
    pos, face, pos_ptr = gref.union([(g.pos, g.face), (i.pos, i.face)])
    ptr = np.array([0, 81, 81 + 128], dtype=np.int64)
    samples = np.concatenate((g.sample_idx, i.sample_idx + 81))
    edges = np.concatenate((g.edges, i.edges + 81))
    perm = np.random.default_rng(5).permutation(len(edges))
    got = log_map_transport(T(pos, dev), T(face, dev), T(samples, dev), T(edges[perm], dev), 0.6, pos_ptr=T(pos_ptr, dev), ptr=T(ptr, dev),
                            return_reached=True)
    # one bound per call: the grid's 0.6 for both meshes
    single_i = log_map_transport(T(i.pos, dev), T(i.face, dev), T(i.sample_idx, dev), T(i.edges, dev), 0.6, return_reached=True)
    for x, a, b in zip(got, device_result('grid'), single_i):
        assert torch.equal(bits(x), bits(torch.cat((a, b))[T(perm, dev)]))
    # host tensors in, host tensors out
    cpu = log_map_transport(torch.from_numpy(g.pos), torch.from_numpy(g.face), torch.from_numpy(g.sample_idx), torch.from_numpy(g.edges), g.bound)
    assert all(not x.is_cuda and torch.equal(bits(x), bits(y).cpu()) for x, y in zip(cpu, device_result('grid')))


@pytest.mark.parametrize('ball_lds', [None, 0])
def test_batch_of_a_mesh_above_the_lds_capacity_and_one_below_equals_single_calls(dev, ball_lds):
    """one call, both instantiations: the 35-vertex lattice relaxes in LDS, the 20 001-vertex strip in global memory, and each takes
    the other's queries for not its own; with ball_lds_vertices = 0 the global instantiation asks for no dynamic LDS at all"""
    from fieldconv_amd.logmap import log_map_transport
    small, strip = gref.lattice(7, 5), case('strip')
    small_samples = np.array([0, 3, 17, 18, 34], dtype=np.int64)
    small_edges, bound = lref.all_pairs(len(small_samples)), strip.bound
    n, s = small[0].shape[0], len(small_samples)
    pos, face, pos_ptr = gref.union([small, (strip.pos, strip.face)])
    ptr = np.array([0, s, s + len(strip.sample_idx)], dtype=np.int64)
    assert pos_ptr[1] == n == 35 and pos_ptr[2] - pos_ptr[1] == 20001 and len(strip.sample_idx) <= 8
    got = log_map_transport(T(pos, dev), T(face, dev), T(np.concatenate((small_samples, strip.sample_idx + n)), dev),
                            T(np.concatenate((small_edges, strip.edges + s)), dev), bound, pos_ptr=T(pos_ptr, dev), ptr=T(ptr, dev),
                            return_reached=True, return_tree=True, ball_lds_vertices=ball_lds)
    a = log_map_transport(T(small[0], dev), T(small[1], dev), T(small_samples, dev), T(small_edges, dev), bound, return_reached=True,
                          return_tree=True)
    b = device_result('strip', tree=True)
    assert bool(a[3].any()) and not bool(a[3].all()) and bool(b[3].any())          # balls stay small: some rows in reach, some not
    for x, y, z in zip(got[:4], a, b):
        assert torch.equal(bits(x), bits(torch.cat((y, z))))
    # the tree: a query's row holds -1 outside its own mesh, and predecessors are vertex numbers of the union
    for k, (x, y, z) in enumerate(zip(got[4:], a[4:], b[4:])):
        off = n if k == 0 else 0
        assert tuple(x.shape) == (s + len(strip.sample_idx), n + 20001)
        assert torch.equal(x[:s, :n], y) and torch.equal(x[s:, n:], torch.where(z >= 0, z + off, z))
        assert bool((x[:s, n:] == -1).all()) and bool((x[s:, :n] == -1).all())


# ------------------------------------------------------------------ 8. determinism
def test_two_runs_give_the_same_bits(dev):
    from fieldconv_amd.logmap import log_map_transport
    c = ico_case()
    args = (T(c.pos, dev), T(c.face, dev), T(c.sample_idx, dev), T(c.edges, dev), c.bound)
    a, b = log_map_transport(*args, return_reached=True, return_tree=True), log_map_transport(*args, return_reached=True, return_tree=True)
    for x, y, z in zip(a, b, device_result('ico', tree=True)):
        assert torch.equal(bits(x), bits(y)) and torch.equal(bits(x), bits(z))


# ------------------------------------------------------------------ 9. end to end
def test_field_conv_on_the_transform_fields(dev):
    """FCPrecomp and one FieldConv forward and backward on ComputeLogXPort's fields and on the float64 restatement's (cast to
    float32): they agree within 4 x what the float32 restatement's fields give against the float64 ones (floor: 1e-6 of the
    largest entry).  The distance from the closed-form sphere's fields is discretisation error: printed, not gated.
    Measured once on an MI355X (also in the README's log-map section): output 7.7e-8 against 7.6e-8 for the float32 restatement's
    fields (largest entry 6.4e-2), the three parameter gradients 3.5e-7, 6.3e-7, 7.5e-8 against 3.4e-7, 6.6e-7, 7.8e-8; the
    closed-form sphere's fields differ by 2.3e-3 in the output and 1.2e-2, 3.3e-2, 5.2e-3 in the gradients."""
    from types import SimpleNamespace
    from fieldconv_amd.nn import FieldConv
    from fieldconv_amd.transforms import ComputeLogXPort, FCPrecomp
    c = ico_case()
    data = SimpleNamespace(pos=T(c.pos, dev), face=T(c.face, dev), sample_idx=T(c.sample_idx, dev), supp_edges=T(c.edges, dev))
    data = ComputeLogXPort(ICO_BOUND)(data)
    assert data.xp.dtype == torch.complex64 and data.logMag.shape == (len(c.edges),) and data.w.shape == (128, 1)
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip((data.logMag, data.logAng, data.xp), device_result('ico')))

    torch.manual_seed(0)
    conv = FieldConv(8, 8, band_limit=2, n_rings=6).to(dev)
    x = torch.randn(128, 8, dtype=torch.complex64).to(dev)
    go = torch.randn(128, 8, dtype=torch.complex64).to(dev)

    def run(mag, ang, xp):
        fields = SimpleNamespace(logMag=mag, logAng=ang, xp=xp, w=data.w, supp_edges=data.supp_edges)
        edges, sten = FCPrecomp(2, 6, 0.9)(fields)[:2]          # 0.9: above every |L|, which a path below the bound cannot exceed
        assert edges.shape[0] == len(c.edges)
        conv.zero_grad()
        out = conv(x, edges, sten)
        out.backward(go)
        return [N_(out)] + [N_(p.grad) for p in conv.parameters() if p.grad is not None]

    def from_ref(L, X):
        mag, ang = lref.polar(L)
        return run(T(mag.astype(np.float32), dev), T(ang.astype(np.float32), dev), T(lref.as_complex(X).astype(np.complex64), dev))
    got = run(data.logMag, data.logAng, data.xp)
    want, own = from_ref(*c.values(np.float64)), from_ref(*c.values(np.float32))
    dist, ang, xp = closed_form(c)
    sphere = run(T(dist.astype(np.float32), dev), T(np.angle(ang).astype(np.float32), dev), T(xp.astype(np.complex64), dev))
    for k, (g, w, o, s) in enumerate(zip(got, want, own, sphere)):
        top = float(np.abs(w).max())
        err, own_err, gate = float(np.abs(g - w).max()), float(np.abs(o - w).max()), max(4 * float(np.abs(o - w).max()), 1e-6 * top)
        print(f'\n{"output" if k == 0 else f"gradient {k}"}: device fields {err:.3e}, float32 restatement fields {own_err:.3e}, gate {gate:.3e}, '
              f'largest entry {top:.3e}; closed-form sphere fields differ by {float(np.abs(s - w).max()):.3e}')
        assert err <= gate
