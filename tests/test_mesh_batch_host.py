"""CPU tests of mesh mini-batches (fieldconv_amd.data.MeshBatch): collation and its inverse on CPU tensors, the offsets, the label
rule, DataLoader collation, and the argument checks that fire before any device work."""
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('pos', 'face', 'sample_idx', 'supp_edges', 'logMag', 'logAng', 'xp', 'w', 'y')


class Mesh:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def make_mesh(n_full, n, k, seed, y='vertex', face=True, pos=True, sample=True):
    g = torch.Generator().manual_seed(seed)
    E = n * k
    src = torch.randint(0, n, (E,), generator=g).sort()[0]
    m = Mesh(supp_edges=torch.stack((src, torch.randint(0, n, (E,), generator=g)), 1), logMag=torch.rand(E, generator=g),
             logAng=torch.rand(E, generator=g), xp=torch.polar(torch.ones(E), torch.rand(E, generator=g)), w=torch.rand(n, 1, generator=g))
    if pos:
        m.pos = torch.randn(n_full, 3, generator=g)
        if face:
            m.face = torch.randint(0, n_full, (3, 2 * n_full), generator=g)
        if sample:
            m.sample_idx = torch.randperm(n_full, generator=g)[:n].sort()[0]
    if y == 'vertex':
        m.y = torch.randint(0, 5, (n,), generator=g)
    elif y == 'scalar':
        m.y = torch.tensor(seed % 5)
    elif y == 'row':
        m.y = torch.tensor([seed % 5])
    elif y == 'vector':
        m.y = torch.rand(3, generator=g)
    return m


def same(a, b):
    names = [k for k in FIELDS if getattr(b, k, None) is not None]
    assert sorted(k for k in FIELDS if getattr(a, k, None) is not None) == sorted(names)
    for k in names:
        assert torch.equal(getattr(a, k), getattr(b, k)) and getattr(a, k).dtype == getattr(b, k).dtype, k


@pytest.mark.parametrize('y', ['vertex', 'scalar', 'row', 'vector', None])
@pytest.mark.parametrize('face,pos,sample', [(True, True, True), (False, True, True), (False, True, False), (False, False, False)])
def test_from_list_then_mesh_is_the_identity(y, face, pos, sample):
    from fieldconv_amd.data import MeshBatch
    sizes = ((50, 20), (31, 31), (9, 1), (120, 64))
    if not sample:
        sizes = tuple((n, n) for _, n in sizes)          # without sample_idx every vertex is a sampled one
    meshes = [make_mesh(nf, n, 3, seed, y=y, face=face, pos=pos, sample=sample) for seed, (nf, n) in enumerate(sizes)]
    batch = MeshBatch.from_list(meshes)
    assert batch.num_meshes == len(batch) == 4
    for b, m in enumerate(meshes):
        same(batch.mesh(b), m)
    with pytest.raises(IndexError):
        batch.mesh(4)
    # .to keeps everything (and is the identity on the same device)
    moved = batch.to('cpu')
    for b, m in enumerate(meshes):
        same(moved.mesh(b), m)


def test_offsets_ranges_and_the_network_input():
    from fieldconv_amd.data import MeshBatch
    meshes = [make_mesh(nf, n, 4, seed) for seed, (nf, n) in enumerate(((40, 10), (25, 25), (70, 33)))]
    batch = MeshBatch.from_list(meshes)
    assert batch.pos_ptr.tolist() == [0, 40, 65, 135] and batch.ptr.tolist() == [0, 10, 35, 68]
    assert batch.edge_ptr.tolist() == [0, 40, 140, 272] and batch.face_ptr.tolist() == [0, 80, 130, 270]
    assert batch.num_nodes == 68 and batch.batch.tolist() == [0] * 10 + [1] * 25 + [2] * 33
    assert batch.pos_ptr.dtype == batch.ptr.dtype == batch.batch.dtype == batch.edge_ptr.dtype == torch.int64
    # data.pos[data.sample_idx] stays the network's input
    assert torch.equal(batch.pos[batch.sample_idx], torch.cat([m.pos[m.sample_idx] for m in meshes]))
    assert torch.equal(batch.pos[batch.face], torch.cat([m.pos[m.face] for m in meshes], 1))
    # edges: offset by ptr, meshes in order, so sources stay sorted and no edge leaves its mesh
    e = batch.supp_edges
    assert torch.equal(e, torch.cat([m.supp_edges + o for m, o in zip(meshes, (0, 10, 35))]))
    assert bool((e[1:, 0] >= e[:-1, 0]).all())
    assert torch.equal(batch.batch[e[:, 0]], batch.batch[e[:, 1]])
    for k in ('logMag', 'logAng', 'xp', 'w'):
        assert torch.equal(getattr(batch, k), torch.cat([getattr(m, k) for m in meshes]))
    assert batch.w.shape == (68, 1)


def test_label_rule():
    from fieldconv_amd.data import MeshBatch
    mk = lambda y: [make_mesh(20, n, 2, seed, y=y) for seed, n in enumerate((5, 8, 3))]
    assert MeshBatch.from_list(mk('vertex')).y.shape == (16,)
    assert MeshBatch.from_list(mk('scalar')).y.tolist() == [0, 1, 2]
    assert MeshBatch.from_list(mk('row')).y.tolist() == [0, 1, 2]              # (1,) labels concatenate to (B,): what cross_entropy takes
    assert MeshBatch.from_list(mk('vector')).y.shape == (3, 3)                  # stacked; not per vertex although one mesh has 3 vertices...
    ms = mk('vertex')
    ms[1].y = torch.tensor([1])
    with pytest.raises(ValueError):
        MeshBatch.from_list(ms)                                                 # per vertex on some meshes, per mesh on another


def test_collate_fn_under_a_dataloader():
    from fieldconv_amd.data import MeshBatch
    meshes = [make_mesh(30 + 3 * i, 10 + i, 3, i, y='row') for i in range(7)]
    loader = torch.utils.data.DataLoader(meshes, batch_size=3, shuffle=False, num_workers=0, collate_fn=MeshBatch.collate_fn)
    batches = list(loader)
    assert [b.num_meshes for b in batches] == [3, 3, 1]
    i = 0
    for batch in batches:
        assert isinstance(batch, MeshBatch) and batch.y.shape == (batch.num_meshes,)
        for b in range(batch.num_meshes):
            same(batch.mesh(b), meshes[i])
            i += 1


def test_a_positions_only_batch_is_what_support_graph_takes():
    from fieldconv_amd.data import MeshBatch
    batch = MeshBatch.from_list([Mesh(pos=torch.rand(n, 3)) for n in (4, 9)])
    assert batch.pos_ptr.tolist() == [0, 4, 13] and batch.ptr is None and batch.supp_edges is None and batch.sample_idx is None
    assert torch.equal(batch.mesh(1).pos, batch.pos[4:])


def test_validation_errors():
    from fieldconv_amd.data import MeshBatch
    good = lambda: [make_mesh(20, 6, 2, 0), make_mesh(15, 9, 2, 1)]
    with pytest.raises(ValueError):
        MeshBatch.from_list([])
    ms = good()
    del ms[1].logAng                                          # missing on one mesh
    with pytest.raises(ValueError):
        MeshBatch.from_list(ms)
    for name, bad in (('supp_edges', torch.zeros(12, 2, dtype=torch.int32)), ('supp_edges', torch.zeros(12, 3, dtype=torch.int64)),
                      ('sample_idx', torch.zeros(6)), ('sample_idx', torch.zeros(5, dtype=torch.int64)), ('pos', torch.zeros(20, 2)),
                      ('pos', torch.zeros(20, 3, dtype=torch.int64)), ('face', torch.zeros(7, 3, dtype=torch.int64)),
                      ('logMag', torch.zeros(11)), ('xp', torch.zeros(13, dtype=torch.complex64)), ('w', torch.zeros(6, 2)),
                      ('w', torch.zeros(7, 1)), ('logAng', [0.0] * 12), ('pos', torch.zeros(20, 3, dtype=torch.float64))):
        ms = good()
        setattr(ms[0], name, bad)
        with pytest.raises(ValueError):
            MeshBatch.from_list(ms)
    with pytest.raises(ValueError):
        MeshBatch.from_list([Mesh(y=torch.tensor(1))])         # nothing to batch
    with pytest.raises(ValueError):
        MeshBatch.from_list([Mesh(pos=torch.rand(4, 3), logMag=torch.rand(3))])          # per-edge data without edges
    ms = good()
    ms[0].pos = ms[0].pos.to('meta')                          # mixed devices, seen without touching a device
    with pytest.raises(ValueError):
        MeshBatch.from_list(ms)


def test_range_tables_are_checked_on_the_host():
    from fieldconv_amd.pooling import check_ptr
    assert check_ptr(torch.tensor([0, 0, 4, 4, 9]), 9, 't') == [0, 0, 4, 4, 9]
    for bad in ([0, 5, 4, 9], [0, 4, 8], [1, 4, 9], [0, 4, 10]):
        with pytest.raises(ValueError):
            check_ptr(torch.tensor(bad), 9, 't')
    for bad in (torch.tensor([0, 9], dtype=torch.int32), torch.tensor([[0, 9]]), torch.tensor([9]), [0, 9]):
        with pytest.raises(ValueError):
            check_ptr(bad, 9, 't')
    # a table that is modified in place is read again
    t = torch.tensor([0, 4, 9])
    check_ptr(t, 9, 't')
    t[1] = 12
    with pytest.raises(ValueError):
        check_ptr(t, 9, 't')


def test_cpu_tensors_raise_and_bad_arguments_come_first(monkeypatch):
    from fieldconv_amd import _lib
    from fieldconv_amd.functional import mesh_mean
    from fieldconv_amd.nn import MeshPool
    from fieldconv_amd.transforms import SupportGraph, farthest_point_sample_batched, radius_edges_batched

    def no_device(*a, **k):
        raise AssertionError('device work attempted')
    monkeypatch.setattr(_lib, 'load', no_device)
    x = torch.zeros(10, 4, dtype=torch.complex64)
    with pytest.raises(RuntimeError):
        MeshPool()(x, torch.tensor([0, 4, 10]))
    with pytest.raises(RuntimeError):
        mesh_mean(torch.zeros(10), torch.tensor([0, 4, 10]))
    with pytest.raises(ValueError):
        MeshPool(reduce='max')
    with pytest.raises(ValueError):
        MeshPool()(torch.zeros(10, 4), torch.tensor([0, 10]))
    pos = torch.rand(10, 3)
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 10]), 5)
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 9]), 1)
    with pytest.raises(ValueError):
        farthest_point_sample_batched(pos, torch.tensor([0, 4, 10]), [1, 2, 3])
    with pytest.raises(ValueError):
        radius_edges_batched(pos, torch.tensor([0, 7, 4, 10]), 0.1)
    with pytest.raises(ValueError):
        radius_edges_batched(pos, torch.tensor([0, 4, 10]), 0.0)
    from fieldconv_amd.data import MeshBatch
    batch = MeshBatch.from_list([Mesh(pos=torch.rand(4, 3)), Mesh(pos=torch.rand(6, 3))])
    batch.sample_idx = torch.arange(10)                       # a preset selection without its ranges
    with pytest.raises(ValueError):
        SupportGraph(0.1)(batch)


def test_public_names():
    from fieldconv_amd import data, nn, transforms
    from fieldconv_amd.functional import mesh_mean, mesh_pool  # noqa: F401
    assert data.__all__[-1] == 'MeshBatch' and nn.__all__[-1] == 'MeshPool'
    assert nn.__all__[:12] == ['TangentNonLin', 'TangentLin', 'TangentPerceptron', 'TransField', 'FieldConv', 'ECHO', 'LiftBlock',
                               'FCResNetBlock', 'ECHOBlock', 'LabelSmoothingLoss', 'TwinLoss', 'TwinEval']
    for name in ('farthest_point_sample_batched', 'radius_edges_batched'):
        assert name in transforms.__all__ and hasattr(transforms, name)


def test_new_modules_never_import_the_oracle_or_torch_geometric():
    for rel in ('data/batch.py', 'pooling.py', 'nn/mesh_pool.py', 'transforms/support_graph.py'):
        src = open(os.path.join(ROOT, 'fieldconv_amd', rel)).read()
        imports = re.findall(r'^\s*(?:from|import)\s+([\w\.]+)', src, flags=re.M)
        assert not any(m.split('.')[0] in ('oracle', 'torch_geometric', 'torch_scatter') for m in imports), rel
