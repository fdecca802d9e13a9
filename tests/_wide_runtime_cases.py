"""Shapes, block arithmetic and GEMM operands for the row-wise tests of the two FieldConv routes that run in pieces: the wide path
(csrc/fc_wide.hip: layers of more than one channel block) and the run-time path (csrc/fc_generic.hip + csrc/fc_cgemm.hip: rings > 8,
band limit > 3 or 0, every complex128 layer).  Inputs, references and the measure are those of _dynamic_range_cases.py (this module
registers its shapes there); test_wide_runtime_host.py pins everything below on the CPU, test_gpu_wide_runtime.py runs the kernels.

The shapes are the smallest at which each mechanism still occurs (N, k, I, O, B, R)."""
import functools

import numpy as np

import _dynamic_range_cases as drc

MAX_BLOCK = 64                  # fieldconv_amd.functional.MAX_CHANNELS: the widest channel block of the compiled kernels
MAX_LDS = 160 * 1024            # csrc/fc_kernels.hpp, kMaxLds: the gather kernel's accumulators of one channel block fit into it

WIDE_SHAPES = {
    'wide129': (200, 10, 129, 65, 1, 3),            # one-channel tail block on both sides, 3 x 2 blocks, ragged last tile
    'wide128': (120, 8, 128, 64, 2, 6),             # exact multiples; one output block (the nob == 1 branch), two input blocks
    'wide_narrow_block': (100, 10, 70, 60, 2, 8),   # _channel_block(...) < 64 at 8 rings
    'wide_split60': (60, 40, 80, 72, 2, 6),         # few tiles, long rows: the edge split inside block launches; tails of 16 and 8
}
# wide129 once more on dense stencil rows: a random stencil that does not factor (mesh: dense_mesh below)
DENSE_SHAPES = {'wide129dense': WIDE_SHAPES['wide129']}
RT_SHAPES = {
    'rt_rings9': (150, 9, 12, 20, 1, 9),            # run-time path on the ring count alone
    'rt_band0': (90, 6, 7, 5, 0, 4),                # F = 1, explicit filter only (the oracle's FCPrecomp does produce B = 0)
    'rt_blocks_f64': (80, 4, 80, 9, 5, 12),         # complex128: 77 + 3 channels in the gather; complex64: one block
    'rt_ksplit': (2100, 4, 6, 5, 1, 9),             # filter-gradient GEMM 5 x 162 over 2100 vertices: split along k
}
SHAPES = {**WIDE_SHAPES, **DENSE_SHAPES, **RT_SHAPES}

# global exponent pairs (names and values of _dynamic_range_cases.GLOBALS)
WIDE_GLOBALS = ('unit-unit', 'tiny-tiny', 'huge-huge', 'unit-tiny', 'huge-unit')
RT_GLOBALS = ('unit-unit', 'tiny-tiny', 'huge-huge')
# (shape, filter type) of the parameter path: wide, and on the run-time path
WIDE_PARAM_CASES = [('wide129', 0), ('wide129', 1), ('wide129', 2), ('wide_narrow_block', 1)]
RT_PARAM_CASES = [('rt_rings9', 1), ('rt_rings9', 2)]


def dense_mesh(name):
    """What drc.mesh returns, for a random stencil without structure (nothing FCPrecomp-like to factor): k random in-edges per
    vertex, a tenth of them dropped, sorted by source; vertex N-2 has no out-edges, vertex 37 no in-edges."""
    N, k, I, O, B, R = SHAPES[name]
    F = 2 * B + 1
    rng = np.random.default_rng([N, k, R, F])
    no_out, no_in = N - 2, 37
    dst = np.repeat(np.arange(N), k)
    src = rng.integers(0, N, N * k)
    keep = (rng.random(N * k) > 0.1) & (src != no_out) & (dst != no_in)
    src, dst = src[keep], dst[keep]
    order = np.argsort(src, kind='stable')
    edges = np.stack((src[order], dst[order]), 1).astype(np.int64)
    E = edges.shape[0]
    sten = ((rng.standard_normal((E, R, F)) + 1j * rng.standard_normal((E, R, F))) * (0.5 / np.sqrt(k))).astype(np.complex64)
    return edges, sten, no_out, no_in


drc.EXTRA_SHAPES.update(SHAPES)
drc.EXTRA_MESHES.update({'wide129dense': dense_mesh})


# ---------------------------------------------------------------- block arithmetic
def blocks(C, blk):
    """[(first channel, width)] of C channels cut into blocks of blk, the last one narrower (csrc/fc_wide.hip)."""
    return [(c0, min(blk, C - c0)) for c0 in range(0, C, blk)]


def gather_block(R, F, itemsize):
    """Input channels per workgroup of fc_generic_gather (csrc/fc_generic.hip, launch_gather): the (R, F) complex accumulators of a
    channel take R F itemsize bytes, and a workgroup's fill the LDS."""
    return MAX_LDS // (R * F * itemsize)


def cgemm_slices(M, N, K, cus):
    """Slices along k of an M x N product over K (csrc/fc_cgemm.hip, cgemm_ksplit) on a device of `cus` compute units."""
    tiles = -(-M // 64) * -(-N // 64)
    slices = 1
    if tiles * 2 <= cus and K >= 2048:
        slices = max(1, min(2 * cus // tiles, (K + 511) // 512, 256))
    per_slice = -(-K // slices)
    chunk = max(16, -(-per_slice // 16) * 16)
    return -(-K // chunk)


# ---------------------------------------------------------------- fc_cgemm: rows scaled by powers of two
# (O, K, n): the filter-gradient product gW (O, K) = G^T conj(A) over n vertices, which is the product the sizes are named after;
# the other two layouts run on the same operands: y (n, O) = A W^T, gC (n, K) = G conj(W)
CGEMM_SIZES = [(5, 162, 2100), (1, 1, 2049), (65, 64, 16), (70, 333, 130)]
CGEMM_A_RANGE = (-20, 13)
CGEMM_G_RANGE = (-10, 10)


@functools.lru_cache(maxsize=None)
def cgemm_case(O, K, n):
    """A (n, K), W (O, K), G (n, O) complex64 with the rows of A and G scaled by powers of two (exactly), and the three products in
    complex128: y = A W^T / 2, gC = G conj(W), gW = 2 G^T conj(A)."""
    rng = np.random.default_rng([O, K, n])
    cplx = lambda *s: (rng.standard_normal(s) + 1j * rng.standard_normal(s)).astype(np.complex64)
    A0, W, G0 = cplx(n, K), cplx(O, K), cplx(n, O)
    a = rng.integers(CGEMM_A_RANGE[0], CGEMM_A_RANGE[1] + 1, n)
    d = rng.integers(CGEMM_G_RANGE[0], CGEMM_G_RANGE[1] + 1, n)
    a[0], d[0] = CGEMM_A_RANGE[1], CGEMM_G_RANGE[1]
    a[-1], d[-1] = CGEMM_A_RANGE[0], CGEMM_G_RANGE[0]
    A = (A0.astype(np.complex128) * np.ldexp(1.0, a)[:, None]).astype(np.complex64)
    G = (G0.astype(np.complex128) * np.ldexp(1.0, d)[:, None]).astype(np.complex64)
    A2, W2, G2 = (t.astype(np.complex128) for t in (A, W, G))
    ref = {'y': A2 @ W2.T * 0.5, 'gC': G2 @ W2.conj(), 'gW': G2.T @ A2.conj() * 2.0}
    for t in (A, W, G, A0, G0, *ref.values()):
        t.setflags(write=False)
    return dict(A=A, W=W, G=G, A0=A0, G0=G0, a=a, d=d, ref=ref)


def rows_and_columns_err(got, ref):
    """(row-wise, column-wise) error of a matrix, both by drc.rowwise_err."""
    got, ref = np.asarray(got).astype(np.complex128), np.asarray(ref)
    return drc.rowwise_err(got, ref), drc.rowwise_err(got.T, ref.T)
