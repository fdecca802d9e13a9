"""Run-time stencil assembly (same call contract as reference transforms/fc_precomp.py:30-97).  Device tensors only, like
every operator of this package.  By default the call goes from the inputs STRAIGHT to the support graph and per-edge
records the convolutions consume (fc_precomp_mark + fc_precomp_graph, csrc/fc_graph.hip) and returns a FactoredStencil in
place of the (E,R,F) tensor -- the dense stencil (154 MB at BASELINE configs[1]) is built only if something asks for it.
FIELDCONV_EAGER_STENCIL=1 keeps the reference's literal outputs (fc_precomp_build)."""
import os

import torch

from .._launch import _po, on as _on, scratch as _scratch, stream as _stream


class FCPrecomp(object):
    """Organises per-edge log-map / transport data into the convolution stencil
    (equations (6)-(7) of the paper).

    data needs: logMag (E), logAng (E), w (N,1), supp_edges (E,2), xp (E complex).
    Returns (supp_edges, supp_sten (E',R,2B+1), ln (E'), wxp (E')) restricted to r <= epsilon.
    """

    def __init__(self, band_limit, n_rings, epsilon):
        self.B = band_limit
        self.R = n_rings
        self.max_r = epsilon
        self._memo = None           # (key of the last inputs, outputs)

    @staticmethod
    def _key(t):
        return (t.data_ptr(), t.storage_offset(), tuple(t.shape), tuple(t.stride()), t._version, str(t.device), t.dtype)

    def __call__(self, data):
        r, theta, w, supp_edges, xp = data.logMag, data.logAng, data.w, data.supp_edges, data.xp
        # The reference runs this in every Net.forward (segmentation.ipynb:202).  The result is a pure function of the
        # five input tensors: when the same (unmodified) tensors come back, e.g. the same mesh in the next epoch, the
        # very same output tensors are returned, so that the support-graph cache keyed on them (graph.get_graph)
        # hits as well instead of re-sorting the edges.
        key = (self.B, self.R, float(self.max_r)) + tuple(self._key(t) for t in (r, theta, w, supp_edges, xp))
        if self._memo is not None and self._memo[0] == key:
            return self._memo[1]
        out = self._compute(r, theta, w, supp_edges, xp)
        self._memo = (key, out, (r, theta, w, supp_edges, xp))      # the inputs are kept alive: their addresses are the key
        return out

    def _compute(self, r, theta, w, supp_edges, xp):
        if not r.is_cuda:
            raise RuntimeError(f'FCPrecomp: fieldconv_amd runs on a ROCm device only (got {r.device} tensors); there is no '
                               'CPU fallback')
        if (r.dtype != torch.float32 or theta.dtype != torch.float32 or w.dtype != torch.float32
                or xp.dtype != torch.complex64):
            raise ValueError('FCPrecomp expects float32 logMag / logAng / w and complex64 xp')
        if self.R < 2 or self.B < 0 or self.R * (2 * self.B + 1) > 156:
            raise ValueError('FCPrecomp supports n_rings >= 2 and band limits >= 0 with n_rings * (2 band_limit + 1) <= 156')
        if r.numel() == 0:
            F = 2 * self.B + 1
            return (supp_edges[:0], torch.zeros((0, self.R, F), dtype=torch.complex64, device=r.device),
                    torch.zeros(0, dtype=torch.complex64, device=r.device), torch.zeros(0, dtype=torch.complex64, device=r.device))
        return self._compute_native(r, theta, w, supp_edges, xp)

    def _compute_native(self, r, theta, w, supp_edges, xp):
        from .. import _lib
        lib = _lib.load()
        dev = r.device
        E, N, R, F = int(r.numel()), int(w.shape[0]), self.R, 2 * self.B + 1
        r, theta, xp = r.contiguous(), theta.contiguous(), xp.contiguous()
        wv = w.reshape(-1).contiguous()
        edges = supp_edges.to(torch.int64).contiguous()
        eps = float(self.max_r)
        with _on(dev):
            st = _stream()
            nbytes = lib.fc_precomp_workspace_bytes(N, E)
            ws = _scratch(nbytes, dev)
            _lib.check(lib.fc_precomp_mark(_po(r), _po(edges), eps, N, E, _po(ws), nbytes, st), 'fc_precomp_mark')
            off = lib.fc_precomp_kept_count_ptr(_po(ws), E) - ws.data_ptr()
            kept, bad = ws[off:off + 8].view(torch.int32).tolist()        # the one synchronisation (the reference's `nonzero`);
            if bad:                                                       # early, while little is queued: the host enqueues
                raise IndexError(f'supp_edges refers to a vertex outside [0, {N})')      # the rest without waiting again
            c64 = dict(dtype=torch.complex64, device=dev)
            edges_out = torch.empty((kept, 2), dtype=torch.int64, device=dev)
            ln, wxp = torch.empty(kept, **c64), torch.empty(kept, **c64)
            if kept == 0:
                return edges_out.to(supp_edges.dtype), torch.zeros((0, R, F), **c64), ln, wxp
            literal = R > 8 or F > 7 or not lib.fc_shape_compiled(R, self.B)     # no record-driven kernels for this shape: the literal (E',R,F) rows
            if literal or os.environ.get('FIELDCONV_EAGER_STENCIL', '0') == '1' or os.environ.get('FIELDCONV_DENSE', '0') == '1':
                sten = torch.empty((kept, R, F), **c64)
                _lib.check(lib.fc_precomp_build(_po(r), _po(theta), _po(xp), _po(wv), _po(edges), eps, N, E, R, F, _po(edges_out), _po(sten), _po(ln),
                                                _po(wxp), _po(ws), nbytes, st), 'fc_precomp_build')
                return edges_out.to(supp_edges.dtype), sten, ln, wxp
            # fused: records and both groupings straight from the inputs
            from ..graph import FactoredStencil, SupportGraph, register_graph
            recf = (4 + 2 * F + 3) // 4 * 4
            want_geo = F >= 3 and os.environ.get('FIELDCONV_NO_GEO', '0') != '1'
            # one allocation for everything the build writes (a dozen separate ones cost more host time than the kernels
            # take on a small mesh); the record arrays get 1 KiB + 16 rows of padding, zero-filled by the build: the kernels
            # stream past the end
            pad_rec, pad_geo = 1024 // (recf * 4) + 16, 1024 // 32 + 16
            sizes = [('rowptr_t', (N + 1,), torch.int32), ('rowptr_s', (N + 1,), torch.int32), ('nbr_t', (kept,), torch.int32),
                     ('nbr_s', (kept,), torch.int32), ('runs_t', (N, 8), torch.int32), ('runs_s', (N, 8), torch.int32),
                     ('perm_t', (kept,), torch.int64), ('perm_s', (kept,), torch.int64), ('factors', (kept, 8), torch.float32),
                     ('flags', (1,), torch.int32), ('rec_t', (kept + pad_rec, recf), torch.float32),
                     ('rec_s', (kept + pad_rec, recf), torch.float32)]
            if want_geo:
                sizes.append(('geo_t', (kept + pad_geo, 8), torch.float32))
            gbytes = lib.fc_graph_workspace_bytes(N, kept, R, F, 1)
            offs, total = {}, 0
            for name, shape, dt in sizes:
                nb = dt.itemsize
                for d in shape:
                    nb *= d
                offs[name] = (total, nb)
                total += (nb + 255) // 256 * 256
            # two allocations: what the graph keeps (views of `arena`) and the build's scratch (edge-order records, keys, ids: ~45 %
            # of the bytes), which goes back to the caching allocator when this call returns instead of staying alive with
            # every cached graph
            arena = torch.empty(total, dtype=torch.uint8, device=dev)
            b = {name: arena[offs[name][0]:offs[name][0] + offs[name][1]].view(dt).view(shape) for name, shape, dt in sizes}
            if not want_geo:
                b['geo_t'] = None
            factors = b['factors']
            gws = _scratch(gbytes, dev)
            _lib.check(lib.fc_precomp_graph(_po(r), _po(theta), _po(xp), _po(wv), _po(edges), eps, N, E, kept, R, F, pad_rec, pad_geo,
                                            _po(edges_out), _po(ln), _po(wxp), _po(factors), _po(b['rowptr_t']), _po(b['nbr_t']), _po(b['runs_t']),
                                            _po(b['perm_t']), _po(b['rowptr_s']), _po(b['nbr_s']), _po(b['runs_s']), _po(b['perm_s']),
                                            _po(b['rec_t']), _po(b['rec_s']), _po(b['geo_t']), _po(b['flags']), _po(ws), nbytes, _po(gws), gbytes, st),
                       'fc_precomp_graph')
        edges_ret = edges_out.to(supp_edges.dtype)
        graph = SupportGraph.from_precomp(edges_ret, N, R, F, b, want_geo)
        sten = FactoredStencil(factors, R, F, graph)
        register_graph(edges_ret, sten, N, graph)
        return edges_ret, sten, ln, wxp

    def __repr__(self):
        return '{}(n_rings={}, epsilon={})'.format(self.__class__.__name__, self.R, self.max_r)
