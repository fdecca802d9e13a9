"""Per-edge log map and parallel transport on the device (csrc/fc_logmap.hip): the xp / logMag / logAng of the reference's
computeLogXPort, by the discrete exponential map of Schmidt, Grimm and Wyvill (2006) over the edge-graph metric of
fieldconv_amd.geodesic.

This is NOT the Vector Heat Method the reference's fcutils solves, and no parity with it is claimed: the layers are
gauge-equivariant, so any consistent choice of frames and transport is a valid input.  What it is instead: restatable.  Per
query sample s the bounded distance field d of geodesic_radius_edges (the same bits on every schedule) fixes a shortest-path
tree by integer and bit decisions only -- edge (u,v) is tight when fl32(d[u] + length) has the bits of d[v]; the hop count h is
the least fixpoint of h[s] = 0, h[v] = 1 + min h[u] over tight edges; pred[v] is the lowest-numbered tight u with
h[u] = h[v] - 1 -- and the tree is unfolded into s's tangent plane by smooth float32 arithmetic:
X[s] = 1, L[s] = 0, X[v] = rho X[u], L[v] = L[u] + conj(X[u]) c (tests/_logmap_ref.py restates all of it in numpy).

Conventions are those of geodesic.py: pos (V,3) float32, face (3,F) int64, on a ROCm device or on the host; the arithmetic
runs on the device either way and results go back to pos's device.  There is no CPU arithmetic path.  Bad arguments raise
ValueError before anything is launched.  Nothing here is differentiable."""
import math

import torch

from . import _lib
from ._launch import on as _on, ptr as _ptr, scratch as _scratch, stream as _stream, whole as _whole
from .geodesic import _batch_tables, _check_diagonals, _check_index, _check_mesh, _face_on, _mesh_on, _prepare, _query_windows

# Reached vertices of one query whose tree state stays in LDS (fc_logmap_ball_lds_vertices: 36 B each, beside the 6 B per
# vertex of the mesh's relaxation state); a larger ball keeps it in a workspace slot, with the same result.
BALL_LDS_VERTICES = 1024
_TREE_ENTRIES = 1 << 24             # return_tree: at most this many (query, vertex) pairs


def _frames(p, f, dev):
    """device tensors in, device tensors out"""
    V, F = int(p.shape[0]), int(f.shape[1])
    lib = _lib.load()
    corner = f.t().reshape(-1)                      # entry 3 f + c: ascending by (face, corner)
    order = torch.sort(corner, stable=True)
    fptr = torch.searchsorted(order.values.contiguous(), torch.arange(V + 1, device=dev)).to(torch.int32)
    fidx = (order.indices // 3).to(torch.int32).contiguous()
    out = torch.empty((3, V, 3), dtype=torch.float32, device=dev)
    _lib.check(lib.fc_vertex_frames(_ptr(p), _ptr(f), _ptr(fptr), _ptr(fidx), V, F, _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), _stream()),
               'fc_vertex_frames')
    return out[0], out[1], out[2]


def vertex_frames(pos, face):
    """(normal, e1, e2), each (V,3) float32: normal[v] is the normalised sum of cross(p1 - p0, p2 - p0) over the faces that
    name v (ascending face order, corners as stored; (0,0,1) where the sum vanishes or v is in no face), e1 =
    normalize(cross(ref, normal)) with ref = (0,0,1) where |normal.z| < 0.95 and (1,0,0) elsewhere, e2 = cross(normal, e1).
    Every operation is a float32 operation rounded on its own.  On the unit sphere with normal = pos these are the frames of
    fieldconv_amd.data.synthetic."""
    what = 'vertex_frames'
    _check_mesh(pos, face, what)
    p, f, dev = _mesh_on(pos, face, what)
    with _on(dev):
        return tuple(t.to(pos.device) for t in _frames(p, f, dev))


def _check_bound(bound, what):
    try:
        ok = not isinstance(bound, bool) and math.isfinite(float(bound)) and float(bound) > 0
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f'{what}: bound must be a finite number > 0, got {bound!r}')
    return float(bound)


def log_map_transport(pos, face, sample_idx, supp_edges, bound, graph=None, pos_ptr=None, ptr=None, return_reached=False, *,
                      return_tree=False, ball_lds_vertices=None, diagonals=False):
    """(logMag (E,) float32, logAng (E,) float32, xp (E,) complex64): for row [a, b] of supp_edges ((E,2) int64 POSITIONS in
    sample_idx, rows in any order; they come back in the caller's order) the polar coordinates of log_a(b) in a's frame, and
    the unit complex number that turns coordinates in a's frame into coordinates in b's frame after transport from a to b: the
    convention of the reference's computeLogXPort, which FCPrecomp consumes.  A row [a, a] gives 0, 0, 1.

    Frames are vertex_frames(pos, face).  Per query a the field d from sample_idx[a] is relaxed while candidates stay below
    fl32(bound) (the field of geodesic_radius_edges), the tree pred is read off its bits (module docstring) and unfolded: for a
    child v of u, c is p_v - p_u without its normal[u] component, in (e1[u], e2[u]), rescaled to the edge's length; rho is e1[u]
    carried by the minimal rotation normal[u] -> normal[v], in v's frame.  X[v] = rho X[u], L[v] = L[u] + conj(X[u]) c; the
    row is |L[t]|, atan2(im L[t], re L[t]) (0 at the origin) and X[t] for t = sample_idx[b].
    A target NOT reached below bound (further away, or in another component) is unfolded as a child of the source over a
    virtual edge of length |p_t - p_s|: the tangent-plane projection.  return_reached: also (E,) bool, False on those rows.
    With GeodesicSupportGraph(epsilon)'s edges and bound = epsilon every row is reached.

    pos_ptr, ptr: both None, or the (B+1,) int64 range tables of a MeshBatch (batch.pos_ptr over pos, batch.ptr over
    sample_idx): a query solves its own mesh only.  graph: mesh_edge_graph(pos, face), to build it once per mesh.
    diagonals: over mesh_edge_graph(pos, face, diagonals=True) (graph must then be None; a graph built with diagonals may be
    passed as graph= as well).  The unfolding step takes any edge (u, v, length): over a diagonal the chord p_v - p_u of the two
    triangles is projected into u's tangent plane and rescaled to the diagonal's unfolded length -- the approximation made for a
    side, applied to a two-triangle chord.
    The two keyword-only arguments serve the tests, not a pipeline.  return_tree (small cases): also pred and hops, (S,V)
    int32 each: per query and vertex of its mesh the predecessor (a vertex number) and the hop count, -1 where there is
    none.  ball_lds_vertices (at most BALL_LDS_VERTICES, the default): balls up to
    this size keep their tree state in LDS, larger ones in a workspace slot; the result does not depend on it.
    One workgroup per query; no atomics, two runs give the same bits."""
    what = 'log_map_transport'
    _check_mesh(pos, face, what)
    _check_diagonals(graph, diagonals, what)
    V = int(pos.shape[0])
    _check_index(sample_idx, V, what, 'sample_idx')
    S = int(sample_idx.numel())
    if not torch.is_tensor(supp_edges) or supp_edges.dim() != 2 or supp_edges.shape[1] != 2 or supp_edges.dtype != torch.int64:
        raise ValueError(f'{what}: supp_edges must be an (E,2) int64 tensor, got '
                         f'{(tuple(supp_edges.shape), supp_edges.dtype) if torch.is_tensor(supp_edges) else type(supp_edges).__name__}')
    R = int(supp_edges.shape[0])
    if R and (int(supp_edges.min()) < 0 or int(supp_edges.max()) >= S):
        raise ValueError(f'{what}: supp_edges must hold positions in sample_idx, in [0, {S})')
    bound = _check_bound(bound, what)
    cap = BALL_LDS_VERTICES if ball_lds_vertices is None else _whole(ball_lds_vertices, 0, BALL_LDS_VERTICES, what, 'ball_lds_vertices',
                                                                     integral_floats=True)
    if return_tree and S * V > _TREE_ENTRIES:
        raise ValueError(f'{what}: return_tree is for small cases, at most {_TREE_ENTRIES} (query, vertex) pairs, got {S} x {V}')
    B, max_range, _, _, tables_on = _batch_tables(pos_ptr, ptr, V, S, what, 'ptr', sample_idx)
    p, f, (gptr, nbr, length), dev = _prepare(pos, face, graph, what, diagonals)
    lib = _lib.load()
    if lib.fc_logmap_ball_lds_vertices() != BALL_LDS_VERTICES:
        raise _lib.FieldConvNativeError(f'{what}: the library keeps {lib.fc_logmap_ball_lds_vertices()} ball vertices in LDS, this module '
                                        f'says {BALL_LDS_VERTICES}: they were built from different sources')
    E_graph = int(nbr.numel())
    per_call, windows = _query_windows(S, lib.fc_logmap_workspace_bytes(max_range, 1, cap))
    with _on(dev):
        nrm, e1, e2 = _frames(p, _face_on(face, V, dev, what) if f is None else f, dev)          # (f is None: graph= was given)
        src = sample_idx.detach().to(dev).contiguous()
        rows = supp_edges.detach().to(dev)
        order = torch.sort(rows[:, 0], stable=True)          # the rows grouped by query
        row_ptr = torch.searchsorted(order.values.contiguous(), torch.arange(S + 1, device=dev))
        target = rows[order.indices, 1].contiguous()
        pp, sp = tables_on(dev)
        nbytes = lib.fc_logmap_workspace_bytes(max_range, per_call, cap)
        ws = _scratch(nbytes, dev, None)
        mag = torch.empty(R, dtype=torch.float32, device=dev)
        ang = torch.empty(R, dtype=torch.float32, device=dev)
        xp = torch.empty((R, 2), dtype=torch.float32, device=dev)
        reached = torch.empty(R, dtype=torch.uint8, device=dev)
        pred = hops = None
        if return_tree:
            pred = torch.full((S, V), -1, dtype=torch.int32, device=dev)
            hops = torch.full((S, V), -1, dtype=torch.int32, device=dev)
        for q0, nq in windows:
            _lib.check(lib.fc_logmap(_ptr(gptr), _ptr(nbr), _ptr(length), V, E_graph, _ptr(pp), _ptr(sp), B, max_range, _ptr(p), _ptr(nrm),
                                     _ptr(e1), _ptr(e2), _ptr(src), S, q0, nq, bound, _ptr(row_ptr), _ptr(target), R,
                                     _ptr(mag), _ptr(ang), _ptr(xp), _ptr(reached), _ptr(pred), _ptr(hops), cap, _ptr(ws), nbytes,
                                     _stream()), 'fc_logmap')
        back = torch.empty_like(order.indices)
        back[order.indices] = torch.arange(R, device=dev)          # the caller's row r is the grouped row back[r]
        out = (mag[back].to(pos.device), ang[back].to(pos.device), torch.view_as_complex(xp[back].contiguous()).to(pos.device))
        if return_reached:
            out += (reached[back].to(torch.bool).to(pos.device),)
        if return_tree:
            out += (pred.to(pos.device), hops.to(pos.device))
    return out
