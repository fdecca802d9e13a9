"""One line per (size query, arguments, value) of the native library's caller-owned buffers, over a fixed grid.

    python tools/workspace_table.py                  # the table, one line per query
    python tools/workspace_table.py --json FILE      # the same lines as a JSON list (tests/golden/workspace_bytes.json)

The queries are host arithmetic: no device is needed and none is used (the process hides them, so a machine with a GPU prints
what a machine without one prints).  A refactor of a layout must leave this table as it is; tests/test_workspace_host.py
compares it with the committed copy."""
import ctypes
import json
import os
import sys

os.environ['HIP_VISIBLE_DEVICES'] = '-1'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NS = (1, 63, 64, 65, 300, 1024, 20000)         # the edges of the per-vertex rules: one chunk, around 64 rows, several workgroups
PARTS = (0, 1, 2)
TOPK = (1, 2, 4, 5, 8)
CONV_NS = (1, 16, 17, 777, 3071, 3072, 4096, 8192, 20000, 170003)
# (I, O, R, B): the channel pairs (1,1) (16,16) (40,48) (48,48) (64,64) (64,48) against the ring / band-limit pairs (2,1) (6,1) (6,2) (6,3)
# (8,3) (5,2), paired so that the reference's default layer (48, 48, 6, 2) is among them; CONV_SHAPES_2: the same lists paired one further
CONV_SHAPES = ((1, 1, 5, 2), (16, 16, 2, 1), (40, 48, 6, 1), (48, 48, 6, 2), (64, 64, 6, 3), (64, 48, 8, 3))
CONV_SHAPES_2 = ((1, 1, 2, 1), (16, 16, 6, 1), (40, 48, 6, 2), (48, 48, 6, 3), (64, 64, 8, 3), (64, 48, 5, 2))
FAKE = 0x10000                                 # a non-null address: the queries test pointers, they never follow these


def rows(lib=None):
    from fieldconv_amd import _lib
    from fieldconv_amd._lib import FcCsr, FcDims, FcEchoBlockParams, FcEchoHeadParams, FcLiftBlockParams, FcMesh, FcResnetBlockParams
    lib = lib or _lib.load()
    out = []

    def q(name, *args, show=None):
        out.append('%s(%s) = %d' % (name, ', '.join(str(a) for a in (show if show is not None else args)), getattr(lib, name)(*args)))

    for N in NS + (0,):
        q('fc_fps_workspace_bytes', N)
        q('fc_fps_batched_workspace_bytes', N)
        q('fc_radius_workspace_bytes', N)
        ptr = lib.fc_radius_edge_count_ptr(ctypes.c_void_p(FAKE), N)
        out.append('fc_radius_edge_count_ptr(ws, %d) - ws = %d' % (N, (ptr or FAKE) - FAKE))
        for E in (0, 1, 12 * N, 100000):
            q('fc_precomp_workspace_bytes', N, E)
        for E in (0, 12 * N):
            for with_sten in (0, 1):
                q('fc_graph_workspace_bytes', N, E, 6, 5, with_sten)
        for K in (7, 32, 33):
            q('fc_label_smoothing_workspace_bytes', N, K)
        for B in (1, 3):
            for C in (5, 64, 100):
                for dt in (0, 1):
                    q('fc_segment_pool_workspace_bytes', N, B, C, dt)
                    q('fc_tangent_norm_workspace_bytes', N, B, C, dt)
        for k in TOPK + (9,):
            for parts in PARTS + (1024, 1025):
                q('fc_match_workspace_bytes', N, k, parts)
        for H, K in ((8, 5), (64, 1000)):
            for parts in PARTS + (64, 65):
                q('fc_linear_ce_workspace_bytes', N, H, K, parts, 0, 0)
                q('fc_linear_ce_workspace_bytes', N, H, K, parts, 1, 0)
                for k in TOPK + (9,):
                    q('fc_linear_ce_workspace_bytes', N, H, K, parts, 2, k)
            q('fc_linear_ce_workspace_bytes', N, H, K, 2, 3, 1)
        for Cin, O, R in ((3, 8, 4), (16, 16, 6), (3, 8, 0)):
            for dt in (0, 1):
                q('fc_trans_field_backward_generic_workspace_bytes', N, Cin, O, R, dt)
            q('fc_trans_field_backward_workspace_bytes', N, Cin, O, R)
        for I, O in ((16, 16), (48, 64)):
            q('fc_tangent_lin_backward_workspace_bytes', N, I, O)
        for C in (16, 64) if N else ():             # (this query takes N >= 1 on trust)
            q('fc_tangent_nonlin_backward_workspace_bytes', N, C)
        for M, K in ((48, 48), (8, 20000)):
            for dt in (0, 1, 2):
                q('fc_cgemm_workspace_bytes', M, N, K, dt)
    for P, M in ((9, 11), (1, 1), (300, 1024), (20000, 20000), (0, 5), (5, 0)):
        q('fc_twin_loss_workspace_bytes', P, M)
    for n_bins in (0, 1, 2, 3, 8, 1024, 1025):
        q('fc_echo_generic_workspace_bytes', n_bins)

    # the dense head: D = 75 keeps the first product whole, D = 4800 splits it on the small N
    for N in NS + (0,):
        for D, H1, H2, C, Q in ((75, 32, 16, 8, 4), (4800, 128, 64, 64, 64), (75, 129, 16, 8, 4)):
            hp = FcEchoHeadParams(D, H1, H2, C, Q)
            show = (N, 'D=%d H1=%d H2=%d C_in=%d C_out=%d' % (D, H1, H2, C, Q))
            q('fc_echo_head_forward_workspace_bytes', N, ctypes.byref(hp), show=show)
            q('fc_echo_head_backward_workspace_bytes', N, ctypes.byref(hp), show=show)

    # whole blocks, per graph kind (0: CSR + stencil, 1 / 2: record streams), and wide layers with a remainder block
    csr = FcCsr(FAKE, FAKE, FAKE)
    for N in NS + (0,):
        for kind in (0, 1, 2, 3):
            mesh = FcMesh(N, 12 * N, 6, 2, kind, ctypes.pointer(csr), ctypes.pointer(csr), FAKE, FAKE, mode=0)
            mshow = 'N=%d E=%d R=6 B=2 kind=%d' % (N, 12 * N, kind)
            for ch in ((16, 32, 48), (64, 64, 64)):
                rp = FcResnetBlockParams(*ch)
                q('fc_resnet_block_saved_bytes', ctypes.byref(mesh), ctypes.byref(rp), show=(mshow, ch))
                for bwd in (0, 1):
                    q('fc_resnet_block_workspace_bytes', ctypes.byref(mesh), ctypes.byref(rp), bwd, show=(mshow, ch, bwd))
            for ch in ((16, 8, 2), (48, 16, 3), (16, 8, 0)):
                ep = FcEchoBlockParams(*ch)
                q('fc_echo_block_saved_bytes', ctypes.byref(mesh), ctypes.byref(ep), show=(mshow, ch))
                for bwd in (0, 1):
                    q('fc_echo_block_workspace_bytes', ctypes.byref(mesh), ctypes.byref(ep), bwd, show=(mshow, ch, bwd))
            for ch in ((3, 16), (16, 48), (0, 16)):
                lp = FcLiftBlockParams(*ch)
                q('fc_lift_block_saved_bytes', ctypes.byref(mesh), ctypes.byref(lp), show=(mshow, ch))
                for bwd in (0, 1):
                    q('fc_lift_block_workspace_bytes', ctypes.byref(mesh), ctypes.byref(lp), bwd, show=(mshow, ch, bwd))
        for I, O in ((112, 104), (128, 64)):
            d = FcDims(N, 12 * N, I, O, 6, 2, mode=0)
            for block in (64, 56, 0, 65):
                for records in (0, 1):
                    for bwd in (0, 1):
                        q('fc_wide_workspace_bytes', ctypes.byref(d), block, records, bwd,
                          show=('N=%d E=%d I=%d O=%d R=6 B=2' % (N, 12 * N, I, O), block, records, bwd))

    # the convolution's own buffers.  Backward: the larger of the pair arrangement (hdump | gwp | gxp) and the streaming one
    # (hrec | gwp | gxt | wst), in each arithmetic mode.  3071 / 3072 vertices sit on the streaming threshold of 256 CUs, 170003 takes
    # the H records past 4 GiB, 40 neighbours at 777 vertices switch the edge split on.
    def conv_rows(N, E, shapes, packed):
        for I, O, R, B in shapes:
            shape = 'N=%d E=%d I=%d O=%d R=%d B=%d' % (N, E, I, O, R, B)
            for mode in (0, 1, 2):
                d = FcDims(N, E, I, O, R, B, mode=mode)
                q('fc_backward_workspace_bytes', ctypes.byref(d), 1, show=(shape + ' mode=%d' % mode, 1))
            d = FcDims(N, E, I, O, R, B, mode=0)
            q('fc_backward_workspace_bytes', ctypes.byref(d), 0, show=(shape, 0))
            q('fc_backward_streams', ctypes.byref(d), 1, show=(shape, 1))
            q('fc_forward_workspace_bytes', ctypes.byref(d), show=(shape,))
            for records in (0, 1) if packed else ():
                q('fc_packed_filter_floats_fwd', ctypes.byref(d), records, show=(shape, records))
                q('fc_packed_filter_floats_bwd', ctypes.byref(d), records, show=(shape, records))

    for N in CONV_NS:
        conv_rows(N, 12 * N, CONV_SHAPES, N in (16, 777, 3072, 20000))
        for O in (1, 16, 48, 64):
            q('fc_tangent_nonlin_backward_workspace_bytes', N, O)
        q('fc_tangent_nonlin_backward_groups', N)
    conv_rows(777, 40 * 777, CONV_SHAPES, False)
    conv_rows(3072, 12 * 3072, CONV_SHAPES_2, False)
    d = FcDims(3072, 12 * 3072, 48, 48, 6, 2, mode=0)
    q('fc_backward_streams', ctypes.byref(d), 0, show=('N=3072 E=36864 I=48 O=48 R=6 B=2', 0))
    for factored in (0, 1):
        q('fc_records_flags', ctypes.byref(d), factored, show=('N=3072 E=36864 I=48 O=48 R=6 B=2', factored))
    return out


if __name__ == '__main__':
    table = rows()
    if len(sys.argv) == 3 and sys.argv[1] == '--json':
        with open(sys.argv[2], 'w') as f:
            json.dump(table, f, indent=0)
            f.write('\n')
    else:
        print('\n'.join(table))
