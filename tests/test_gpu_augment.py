"""Per-mesh augmentation on the device (fieldconv_amd.augment, csrc/fc_augment.hip, transforms.RandomMeshAffine) against the numpy
restatement tests/_philox_ref.py.

params (scale and angles) and the affine map are chains of separately rounded float32 operations and are compared BIT FOR BIT.  The
matrices go through the device library's sinf and cosf: they are compared against the float64 restatement built from the same
float32 params, within max(4 x the float32 restatement's own error, 1e-6 x the largest entry)."""
import numpy as np
import pytest
import torch

import _philox_ref as pref

pytestmark = pytest.mark.gpu

SEED = 2024
PTR = [0, 1, 5, 14]          # three meshes of 1, 4 and 9 vertices


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available(), 'needs a ROCm device'
    return torch.device('cuda:0')


def T(a, dev=torch.device('cuda:0')):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def N_(t):
    return t.detach().cpu().numpy()


def same(got, want):
    """bit for bit outside NaN rows, NaN where NaN is wanted"""
    if got.dtype != want.dtype or got.shape != want.shape or not np.array_equal(np.isnan(got), np.isnan(want)):
        return False
    ok = ~np.isnan(want)
    return np.array_equal(np.ascontiguousarray(got[ok]).view(np.uint32), np.ascontiguousarray(want[ok]).view(np.uint32))


def positions(V, salt=0):
    return np.random.default_rng(77 + salt).uniform(-1.0, 1.0, (V, 3)).astype(np.float32)


def device_ptr(dev, ptr=PTR):
    from fieldconv_amd.pooling import tag_ptr
    return tag_ptr(torch.tensor(ptr, dtype=torch.int64).to(dev), ptr)


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize('scale', [None, (0.85, 1.15)], ids=['no-scale', 'scale'])
@pytest.mark.parametrize('B', [1, 5])
def test_draw(dev, B, scale):
    from fieldconv_amd.functional import random_mesh_affine
    degrees = (45, 30, 15)
    for step in (0, 7, torch.tensor([7], dtype=torch.int64, device=dev)):
        params, M = random_mesh_affine(B, SEED, step, scale, degrees, device=dev)
        want = pref.affine_params(B, SEED, int(step), scale, degrees)
        assert params.dtype == torch.float32 and tuple(params.shape) == (B, 4) and tuple(M.shape) == (B, 3, 3)
        assert same(N_(params), want), step                                  # exact: separately rounded float32 operations
        M64, M32 = pref.affine_matrix(want, np.float64), pref.affine_matrix(want, np.float32)
        own = float(np.abs(M32 - M64).max())
        err = float(np.abs(N_(M) - M64).max())
        gate = max(4 * own, 1e-6 * float(np.abs(M64).max()))
        print(f'\nB={B} scale={scale} step={int(step)}: device M against float64 {err:.3e}, float32 restatement {own:.3e}, gate {gate:.3e}')
        assert np.isfinite(N_(M)).all() and err <= gate, (err, gate)
        assert (np.linalg.det(N_(M).astype(np.float64)) > 0).all()
    if scale is None:
        assert (N_(params)[:, 0] == 1).all()
    a, _ = random_mesh_affine(B, SEED, 0, scale, degrees, device=dev)
    b, _ = random_mesh_affine(B, SEED, 1, scale, degrees, device=dev)
    assert not same(N_(a), N_(b))                                            # two steps differ


# ------------------------------------------------------------------ the affine map
@pytest.mark.parametrize('indexed', [False, True], ids=['all', 'index'])
@pytest.mark.parametrize('centred', [False, True], ids=['no-t', 't'])
def test_apply_equals_the_restatement_bit_for_bit(dev, centred, indexed):
    from fieldconv_amd.functional import mesh_affine, mesh_mean, random_mesh_affine
    pos = positions(PTR[-1])
    pos_d, ptr_d = T(pos, dev), device_ptr(dev)
    before = pos_d.clone()
    _, M = random_mesh_affine(3, SEED, 2, (0.85, 1.15), device=dev)
    t = mesh_mean(pos_d, ptr_d) if centred else None
    index = np.array([13, 0, 4, 14, 1, 5, 5, -1, 12], dtype=np.int64) if indexed else None          # 14 and -1 lie outside [0, 14)
    out = mesh_affine(pos_d, ptr_d, M, t, None if index is None else T(index, dev))
    want = pref.affine_apply(pos, PTR, N_(M), None if t is None else N_(t), index)
    assert out.data_ptr() != pos_d.data_ptr() and torch.equal(pos_d, before)          # a new tensor; pos is not written
    assert same(N_(out), want)
    if indexed:
        assert np.isnan(N_(out)[[3, 7]]).all() and np.isfinite(np.delete(N_(out), [3, 7], axis=0)).all()
        assert tuple(mesh_affine(pos_d, ptr_d, M, t, torch.empty(0, dtype=torch.int64, device=dev)).shape) == (0, 3)
    if centred and not indexed:                                              # centred on each mesh's own mean
        for b in range(3):
            mean = N_(out)[PTR[b]:PTR[b + 1]].astype(np.float64).mean(0)
            assert np.abs(mean).max() <= 1e-6


def test_more_rows_than_one_workgroup(dev):
    from fieldconv_amd.functional import mesh_affine, random_mesh_affine
    ptr = [0, 300, 300, 1000]                                                # an empty mesh; 1000 rows: four workgroups
    pos = positions(1000, 1)
    _, M = random_mesh_affine(3, SEED, 0, device=dev)
    t = positions(3, 2)
    index = np.random.default_rng(5).integers(0, 1000, 777)
    out = mesh_affine(T(pos, dev), torch.tensor(ptr), M, T(t, dev), T(index, dev))          # (a host table is moved)
    assert same(N_(out), pref.affine_apply(pos, ptr, N_(M), t, index))
    assert same(N_(mesh_affine(T(pos, dev), device_ptr(dev, ptr), M)), pref.affine_apply(pos, ptr, N_(M)))


# ------------------------------------------------------------------ the transform
class Mesh:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_batch(dev):
    from fieldconv_amd.data import MeshBatch
    meshes = []
    for b in range(3):
        V = PTR[b + 1] - PTR[b]
        n = max(1, V // 2)
        E = 2 * n
        g = torch.Generator().manual_seed(b)
        meshes.append(Mesh(pos=torch.from_numpy(positions(V, 10 + b)), sample_idx=torch.randperm(V, generator=g)[:n],
                           supp_edges=torch.randint(0, n, (E, 2), generator=g), logMag=torch.rand(E, generator=g),
                           logAng=torch.rand(E, generator=g), xp=torch.rand(E, generator=g), w=torch.rand(n, 1, generator=g)))
    return MeshBatch.from_list(meshes).to(dev)


def test_transform_on_a_batch_equals_its_draw_applied_mesh_by_mesh(dev):
    from fieldconv_amd.functional import mesh_affine, mesh_mean, random_mesh_affine
    from fieldconv_amd.norm import whole_ptr
    from fieldconv_amd.transforms import RandomMeshAffine
    scale, degrees = (0.85, 1.15), (45, 30, 15)
    batch = make_batch(dev)
    pos0, before = batch.pos, batch.pos.clone()
    kept = {k: getattr(batch, k) for k in ('logMag', 'logAng', 'xp', 'w', 'supp_edges', 'sample_idx', 'pos_ptr', 'ptr', 'edge_ptr')}
    aug = RandomMeshAffine(scale=scale, degrees=degrees, center=True, seed=SEED)
    for step in range(2):
        batch.pos = pos0
        out = aug(batch)
        assert out is batch and batch.pos is not pos0 and torch.equal(pos0, before)          # the caller's tensor is not written
        assert all(getattr(batch, k) is v for k, v in kept.items())                          # the precomputed fields: the same objects
        assert int(aug.step) == step + 1 and aug.step.device == pos0.device
        _, M = random_mesh_affine(3, SEED, step, scale, degrees, device=dev)
        for b in range(3):
            pb = pos0[PTR[b]:PTR[b + 1]]
            one = whole_ptr(pb.shape[0], dev)
            alone = mesh_affine(pb, one, M[b:b + 1], mesh_mean(pb, one))
            assert same(N_(batch.pos[PTR[b]:PTR[b + 1]]), N_(alone)), (step, b)
    first = RandomMeshAffine(scale=scale, degrees=degrees, center=True, seed=SEED)
    batch.pos = pos0
    assert not same(N_(first(batch).pos), N_(aug(Mesh(pos=pos0, pos_ptr=batch.pos_ptr)).pos))          # step 0 against step 2


def test_input_equals_the_transformed_positions_of_the_samples(dev):
    from fieldconv_amd.transforms import RandomMeshAffine
    for kw in (dict(scale=(0.85, 1.15), center=True), dict()):
        batch = make_batch(dev)
        pos0 = batch.pos
        a, b = RandomMeshAffine(seed=SEED, **kw), RandomMeshAffine(seed=SEED, **kw)
        x = a.input(batch)
        assert batch.pos is pos0 and tuple(x.shape) == (batch.sample_idx.shape[0], 3) and int(a.step) == 1
        moved = b(batch)
        assert same(N_(x), N_(moved.pos[batch.sample_idx]))
    with pytest.raises(ValueError):
        RandomMeshAffine(seed=SEED).input(Mesh(pos=pos0))


def test_a_single_mesh_is_a_batch_of_one(dev):
    from fieldconv_amd.transforms import RandomMeshAffine
    pos = positions(9, 3)
    mesh = Mesh(pos=T(pos, dev))
    out = RandomMeshAffine(scale=(0.5, 2.0), seed=SEED)(mesh)
    params = pref.affine_params(1, SEED, 0, (0.5, 2.0))
    want = pref.affine_apply(pos, [0, 9], pref.affine_matrix(params, np.float64).astype(np.float32))
    # (the device's own M differs from the restated one in the last place: a tolerance, here only)
    assert out is mesh and np.abs(N_(mesh.pos) - want).max() <= 1e-5
    lengths = np.linalg.norm(N_(mesh.pos).astype(np.float64), axis=1) / np.linalg.norm(pos.astype(np.float64), axis=1)
    assert np.abs(lengths - float(params[0, 0])).max() <= 1e-5                # a similarity: every length scaled by s
