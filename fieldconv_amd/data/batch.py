"""Mini-batches of meshes: the disjoint union of several meshes as ONE mesh of the package's data contract.

The convolutions, FCPrecomp and the blocks need nothing new for a batch -- a disjoint union is just a graph, and FCPrecomp's
weight normalisation is per target vertex -- so MeshBatch only builds the union (indices offset, ranges recorded) and hands it
on: FCPrecomp(...)(batch) returns the union's (supp_edges, supp_sten, ln, wxp), the blocks take them as they take a single
mesh's, and MeshPool / mesh_mean (fieldconv_amd.nn, fieldconv_amd.functional) reduce per mesh at the end.  Works on CPU
tensors (where a DataLoader collates) and on device tensors; everything is sized from tensor SHAPES, so building a batch
never synchronises with a device.  No torch_geometric."""
import torch

from ..pooling import ptr_host, tag_ptr
from .synthetic import SupportData

_PER_EDGE = ('logMag', 'logAng', 'xp')
_KNOWN = ('pos', 'face', 'sample_idx', 'supp_edges', 'logMag', 'logAng', 'xp', 'w', 'y')


def _table(counts, device):
    host = [0]
    for c in counts:
        host.append(host[-1] + int(c))
    return tag_ptr(torch.tensor(host, dtype=torch.int64).to(device), host)


def _offsets(counts, starts, device):
    """(sum counts,) int64: starts[b] repeated counts[b] times"""
    return torch.repeat_interleave(torch.tensor(list(starts), dtype=torch.int64), torch.tensor(list(counts), dtype=torch.int64)).to(device)


class MeshBatch(object):
    """The union of B meshes, built by MeshBatch.from_list(meshes).  Each mesh is any object with the attributes the transforms
    and FCPrecomp use; every attribute is either present on all meshes or on none:

        pos (n_full,3), face (3,F)              full-resolution vertices and triangles (optional)
        sample_idx (n,)                         the sampled vertices among pos (optional)
        supp_edges (E,2), logMag, logAng, xp (E), w (n,1)      the support graph and its per-edge / per-vertex fields
        y                                       labels: per vertex when y.shape[0] == n, otherwise one per mesh

    The batch carries the same names for the union, plus the ranges:

        pos, pos_ptr (B+1)                      positions concatenated; mesh b owns pos[pos_ptr[b]:pos_ptr[b+1]]
        face, sample_idx                        offset by pos_ptr: batch.pos[batch.sample_idx] stays the network's input;
        face_ptr (B+1)                          mesh b owns face[:, face_ptr[b]:face_ptr[b+1]]
        ptr (B+1), batch (N,), num_meshes       ranges of the SAMPLED vertices (n = rows of w, else of sample_idx, else of pos when
                                                the mesh has supp_edges), and each sampled vertex's mesh
        supp_edges, edge_ptr (B+1)              offset by ptr, meshes in order (each mesh's source-sorted edge order is kept)
        logMag, logAng, xp, w                   concatenated
        y                                       per-vertex labels concatenated; per-mesh labels one row per mesh: scalars and
                                                (1, ...) labels concatenate to (B, ...), anything else is stacked

    A batch of meshes that have only pos (and face) is what SupportGraph takes to build sample_idx, ptr, batch and supp_edges
    for all meshes at once.  .to(device) moves every tensor; .mesh(b) gives the b-th mesh back with the offsets removed
    (from_list followed by mesh(b) is the identity)."""

    def __init__(self):
        for name in _KNOWN + ('pos_ptr', 'face_ptr', 'ptr', 'batch', 'edge_ptr'):
            setattr(self, name, None)
        self.num_meshes = 0
        self._y_kind = None

    # ------------------------------------------------------------------ construction
    @classmethod
    def from_list(cls, meshes):
        meshes = list(meshes)
        if not meshes:
            raise ValueError('MeshBatch.from_list: no meshes')
        B = len(meshes)
        have = {}
        for name in _KNOWN:
            vals = [getattr(m, name, None) for m in meshes]
            present = [v is not None for v in vals]
            if any(present) and not all(present):
                raise ValueError(f'MeshBatch.from_list: {name} is missing on mesh {present.index(False)} but present on others')
            if all(present):
                for i, v in enumerate(vals):
                    if not torch.is_tensor(v):
                        raise ValueError(f'MeshBatch.from_list: {name} of mesh {i} must be a tensor, got {type(v).__name__}')
                have[name] = vals
        if 'pos' not in have and 'supp_edges' not in have:
            raise ValueError('MeshBatch.from_list: the meshes need pos, or supp_edges with logMag, logAng, xp and w')
        devices = {v.device for vals in have.values() for v in vals}
        if len(devices) != 1:
            raise ValueError(f'MeshBatch.from_list: tensors on mixed devices {sorted(str(d) for d in devices)}')
        dev = devices.pop()
        self = cls()
        self.num_meshes = B

        if 'pos' in have:
            for i, p in enumerate(have['pos']):
                if p.dim() != 2 or p.shape[1] != 3 or not p.is_floating_point():
                    raise ValueError(f'MeshBatch.from_list: pos of mesh {i} must be an (n,3) floating-point tensor, got {tuple(p.shape)} {p.dtype}')
            if len({p.dtype for p in have['pos']}) != 1:
                raise ValueError('MeshBatch.from_list: pos dtypes differ between meshes')
            n_full = [int(p.shape[0]) for p in have['pos']]
            self.pos = torch.cat(have['pos'], 0)
            self.pos_ptr = _table(n_full, dev)
        elif 'face' in have or 'sample_idx' in have:
            raise ValueError('MeshBatch.from_list: face / sample_idx index pos, which the meshes do not have')
        pos_starts = ptr_host(self.pos_ptr, 'MeshBatch')[:-1] if self.pos_ptr is not None else None

        if 'face' in have:
            for i, f in enumerate(have['face']):
                if f.dim() != 2 or f.shape[0] != 3 or f.dtype != torch.int64:
                    raise ValueError(f'MeshBatch.from_list: face of mesh {i} must be a (3,F) int64 tensor, got {tuple(f.shape)} {f.dtype}')
            n_faces = [int(f.shape[1]) for f in have['face']]
            self.face = torch.cat(have['face'], 1) + _offsets(n_faces, pos_starts, dev)[None, :]
            self.face_ptr = _table(n_faces, dev)
        if 'sample_idx' in have:
            for i, s in enumerate(have['sample_idx']):
                if s.dim() != 1 or s.dtype != torch.int64:
                    raise ValueError(f'MeshBatch.from_list: sample_idx of mesh {i} must be an (n,) int64 tensor, got {tuple(s.shape)} {s.dtype}')
            self.sample_idx = torch.cat(have['sample_idx'], 0) + _offsets([s.shape[0] for s in have['sample_idx']], pos_starts, dev)

        # sampled vertices per mesh
        n = None
        if 'w' in have:
            for i, w in enumerate(have['w']):
                if w.dim() not in (1, 2) or (w.dim() == 2 and w.shape[1] != 1) or not w.is_floating_point():
                    raise ValueError(f'MeshBatch.from_list: w of mesh {i} must be an (n,1) floating-point tensor, got {tuple(w.shape)} {w.dtype}')
            if len({(w.dim(), w.dtype) for w in have['w']}) != 1:
                raise ValueError('MeshBatch.from_list: w shapes / dtypes differ between meshes')
            n = [int(w.shape[0]) for w in have['w']]
            self.w = torch.cat(have['w'], 0)
        if 'sample_idx' in have:
            ns = [int(s.shape[0]) for s in have['sample_idx']]
            if n is not None and n != ns:
                raise ValueError(f'MeshBatch.from_list: w has {n} rows per mesh but sample_idx selects {ns} vertices')
            n = ns
        if n is None and 'supp_edges' in have:
            n = [int(p.shape[0]) for p in have['pos']] if 'pos' in have else None
            if n is None:
                raise ValueError('MeshBatch.from_list: the number of sampled vertices is unknown: give w or sample_idx with supp_edges')
        if n is not None:
            self._set_ranges(n, dev)

        if 'supp_edges' in have:
            for i, e in enumerate(have['supp_edges']):
                if e.dim() != 2 or e.shape[1] != 2 or e.dtype != torch.int64:
                    raise ValueError(f'MeshBatch.from_list: supp_edges of mesh {i} must be an (E,2) int64 tensor, got {tuple(e.shape)} {e.dtype}')
            n_edges = [int(e.shape[0]) for e in have['supp_edges']]
            starts = ptr_host(self.ptr, 'MeshBatch')[:-1]
            self.supp_edges = torch.cat(have['supp_edges'], 0) + _offsets(n_edges, starts, dev)[:, None]
            self.edge_ptr = _table(n_edges, dev)
            for name in _PER_EDGE:
                if name not in have:
                    continue
                for i, v in enumerate(have[name]):
                    if v.dim() != 1 or v.shape[0] != n_edges[i]:
                        raise ValueError(f'MeshBatch.from_list: {name} of mesh {i} must be ({n_edges[i]},) like its supp_edges, got {tuple(v.shape)}')
                if len({v.dtype for v in have[name]}) != 1:
                    raise ValueError(f'MeshBatch.from_list: {name} dtypes differ between meshes')
                setattr(self, name, torch.cat(have[name], 0))
        else:
            for name in _PER_EDGE:
                if name in have:
                    raise ValueError(f'MeshBatch.from_list: {name} is per edge, but the meshes have no supp_edges')

        if 'y' in have:
            ys = have['y']
            if n is not None and all(y.dim() >= 1 and y.shape[0] == nb for y, nb in zip(ys, n)):
                self._y_kind, self.y = 'vertex', torch.cat(ys, 0)
            elif len({(tuple(y.shape), y.dtype) for y in ys}) != 1:
                # (labels of one shape whose length happens to equal one mesh's vertex count are per-mesh labels)
                raise ValueError('MeshBatch.from_list: y must be per vertex on every mesh, or one label of the same shape and dtype per mesh')
            elif ys[0].dim() == 0:
                self._y_kind, self.y = 'scalar', torch.stack(ys, 0)
            elif ys[0].shape[0] == 1:
                self._y_kind, self.y = 'row', torch.cat(ys, 0)
            else:
                self._y_kind, self.y = 'stack', torch.stack(ys, 0)
        return self

    def _set_ranges(self, n, device):
        """ptr, batch from the sampled-vertex counts (Python ints)"""
        self.ptr = _table(n, device)
        self.batch = _offsets(n, range(len(n)), device)

    collate_fn = None          # (set below: a plain function, so that DataLoader(collate_fn=MeshBatch.collate_fn) works)

    # ------------------------------------------------------------------ the data contract
    @property
    def num_nodes(self):
        return None if self.ptr is None else ptr_host(self.ptr, 'MeshBatch')[-1]

    def _tensors(self):
        return [k for k in _KNOWN + ('pos_ptr', 'face_ptr', 'ptr', 'batch', 'edge_ptr') if getattr(self, k) is not None]

    def to(self, device):
        out = MeshBatch()
        out.num_meshes, out._y_kind = self.num_meshes, self._y_kind
        for k in self._tensors():
            src = getattr(self, k)
            dst = src.to(device)
            memo = getattr(src, '_fc_ptr_host', None)
            if memo is not None and dst is not src and memo[0] == src._version:
                tag_ptr(dst, memo[1])
            setattr(out, k, dst)
        return out

    def mesh(self, b):
        """The b-th mesh with its own numbering (a SupportData attribute bag).  Reads the range tables on the host: free for a
        batch built by from_list, one read-back for tables computed on the device (SupportGraph's edge_ptr)."""
        if isinstance(b, bool) or int(b) != b or not 0 <= b < self.num_meshes:
            raise IndexError(f'MeshBatch.mesh: mesh {b!r} of {self.num_meshes}')
        b = int(b)
        out = {}
        p0 = p1 = None
        if self.pos is not None:
            pp = ptr_host(self.pos_ptr, 'MeshBatch.mesh', 'pos_ptr')
            p0, p1 = pp[b], pp[b + 1]
            out['pos'] = self.pos[p0:p1]
        if self.face is not None:
            fp = ptr_host(self.face_ptr, 'MeshBatch.mesh', 'face_ptr')
            out['face'] = self.face[:, fp[b]:fp[b + 1]] - p0
        v0 = v1 = None
        if self.ptr is not None:
            vp = ptr_host(self.ptr, 'MeshBatch.mesh')
            v0, v1 = vp[b], vp[b + 1]
            if self.sample_idx is not None:
                out['sample_idx'] = self.sample_idx[v0:v1] - p0
            if self.w is not None:
                out['w'] = self.w[v0:v1]
        if self.supp_edges is not None:
            ep = ptr_host(self.edge_ptr, 'MeshBatch.mesh', 'edge_ptr')
            e0, e1 = ep[b], ep[b + 1]
            out['supp_edges'] = self.supp_edges[e0:e1] - v0
            for name in _PER_EDGE:
                if getattr(self, name) is not None:
                    out[name] = getattr(self, name)[e0:e1]
        if self.y is not None:
            out['y'] = {'vertex': lambda: self.y[v0:v1], 'scalar': lambda: self.y[b], 'row': lambda: self.y[b:b + 1],
                        'stack': lambda: self.y[b]}[self._y_kind]()
        return SupportData(**out)

    def __len__(self):
        return self.num_meshes

    def __repr__(self):
        return 'MeshBatch(num_meshes={}, {})'.format(self.num_meshes, ', '.join(
            '{}={}'.format(k, list(getattr(self, k).shape)) for k in self._tensors()))


def collate_fn(meshes):
    """torch.utils.data.DataLoader(dataset, batch_size=B, collate_fn=MeshBatch.collate_fn): a list of meshes -> one MeshBatch"""
    return MeshBatch.from_list(meshes)


MeshBatch.collate_fn = staticmethod(collate_fn)
