"""numpy restatements of the counter-based generator (csrc/fc_philox.hpp) and of its two users: the dropout masks and values
(csrc/fc_dropout.hip) and the per-mesh augmentation (csrc/fc_augment.hip).  Philox4x32-10 as published (Salmon et al., SC'11;
Random123): nothing here is taken from another implementation.  Everything an integer or a chain of separately rounded float32
operations is restated bit for bit; the rotation matrices go through sin / cos and come in float32 and in float64."""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)
SHIFT32 = np.uint64(32)
ELEMENT, CHANNEL, AUGMENT = 0, 1, 2          # the streams

# the published known-answer vectors of Philox4x32-10: (counter, key, expected words)
KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two ints -> (n,4) uint64 array of 32-bit words.  Ten rounds of
    p0 = M0 * c0, p1 = M1 * c2 (64-bit products), c = (hi(p1) ^ c1 ^ k0, lo(p1), hi(p0) ^ c3 ^ k1, lo(p0)), key bumped after each."""
    c0, c1, c2, c3 = (np.atleast_1d(np.asarray(c, dtype=np.uint64)) & MASK32 for c in np.broadcast_arrays(*counter))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2          # (below 2^64: no wrap)
        c0, c1, c2, c3 = (p1 >> SHIFT32) ^ c1 ^ np.uint64(k0), p1 & MASK32, (p0 >> SHIFT32) ^ c3 ^ np.uint64(k1), p0 & MASK32
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=1)


def words(seed, hi, first_block, n_blocks):
    """fc_philox_words: (n_blocks, 4), block i of the counter (lo32(q), hi32(q), lo32(hi), hi32(hi)), q = first_block + i mod 2^64"""
    q = np.array([(int(first_block) + i) % 2 ** 64 for i in range(n_blocks)], dtype=np.uint64)
    return philox4x32_10((q & MASK32, q >> SHIFT32, int(hi) & 0xFFFFFFFF, int(hi) >> 32), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))


def draw_blocks(seed, q, step, stream):
    """the package's convention: key (lo32(seed), hi32(seed)), counter (lo32(q), hi32(q), lo32(step), stream)"""
    q = np.atleast_1d(np.asarray(q, dtype=np.uint64))
    return philox4x32_10((q & MASK32, q >> SHIFT32, int(step) & 0xFFFFFFFF, int(stream)), (int(seed) & 0xFFFFFFFF, int(seed) >> 32))


def bits24(seed, step, stream, e):
    """the 24 bits of entry e of a draw: word e & 3 of block e >> 2, shifted right by 8"""
    e = np.asarray(e, dtype=np.uint64)
    flat = e.reshape(-1)
    q, where = np.unique(flat >> np.uint64(2), return_inverse=True)          # (each block once: four entries share one)
    w = draw_blocks(seed, q, step, stream)[where.reshape(-1), (flat & np.uint64(3)).astype(np.int64)]
    return (w >> np.uint64(8)).reshape(e.shape)


def threshold(p):
    return int(float(p) * float(1 << 24))


def element_keep(N, C, p, seed, step):
    """(N,C) bool, True where the entry is KEPT: e = n C + c, dropped iff bits24 < floor(p 2^24)"""
    e = np.arange(N * C, dtype=np.uint64).reshape(N, C)
    return bits24(seed, step, ELEMENT, e) >= np.uint64(threshold(p))


def channel_keep(ptr, C, p, seed, step):
    """(N,C) bool: one decision per mesh and channel, e = b C + c, shared by the rows ptr[b] .. ptr[b+1] - 1"""
    B = len(ptr) - 1
    per_mesh = bits24(seed, step, CHANNEL, np.arange(B * C, dtype=np.uint64).reshape(B, C)) >= np.uint64(threshold(p))
    mesh_of_row = np.repeat(np.arange(B), np.diff(np.asarray(ptr)))
    return per_mesh[mesh_of_row].reshape(int(ptr[-1]), C)


def dropout(x, keep, p):
    """kept: scale * x with scale = 1 / (1 - p) in double, rounded once to x's real type, re and im each; dropped: +0"""
    real = x.real.dtype
    scale = real.type(1.0 / (1.0 - float(p)))
    if np.iscomplexobj(x):
        y = np.zeros_like(x)
        y.real = np.where(keep, x.real * scale, real.type(0))
        y.imag = np.where(keep, x.imag * scale, real.type(0))
        return y
    return np.where(keep, x * scale, real.type(0)).astype(x.dtype)


def uniforms(seed, step, stream, e):
    """u = (word >> 8) * 2^-24: exact in float32, in [0, 1)"""
    return bits24(seed, step, stream, e).astype(np.float32) * np.float32(2.0 ** -24)


def affine_params(B, seed, step, scale=None, degrees=(45, 45, 45)):
    """(B,4) float32 (s, a_0, a_1, a_2): mesh b draws from block b of stream 2; every operation a float32 operation"""
    u = uniforms(seed, step, AUGMENT, np.arange(4 * B, dtype=np.uint64).reshape(B, 4))
    out = np.empty((B, 4), dtype=np.float32)
    if scale is None:
        out[:, 0] = 1
    else:
        lo, hi = np.float32(scale[0]), np.float32(scale[1])
        out[:, 0] = lo + (hi - lo) * u[:, 0]
    for k in range(3):
        out[:, 1 + k] = (np.float32(2) * u[:, 1 + k] - np.float32(1)) * np.float32(degrees[k])
    return out


def affine_matrix(params, dtype):
    """(B,3,3) of dtype: s Rz(r_2) Ry(r_1) Rx(r_0), r_k = a_k * fl32(pi / 180), from the float32 params, all arithmetic in dtype"""
    p = np.asarray(params, dtype=np.float32).astype(dtype)
    rad = dtype(np.float32(np.pi / 180))
    out = np.empty((p.shape[0], 3, 3), dtype=dtype)
    for b in range(p.shape[0]):
        s, (r0, r1, r2) = p[b, 0], p[b, 1:] * rad
        cx, sx, cy, sy, cz, sz = np.cos(r0), np.sin(r0), np.cos(r1), np.sin(r1), np.cos(r2), np.sin(r2)
        one, zero = dtype(1), dtype(0)
        Rx = np.array([[one, zero, zero], [zero, cx, -sx], [zero, sx, cx]], dtype=dtype)
        Ry = np.array([[cy, zero, sy], [zero, one, zero], [-sy, zero, cy]], dtype=dtype)
        Rz = np.array([[cz, -sz, zero], [sz, cz, zero], [zero, zero, one]], dtype=dtype)
        out[b] = s * (Rz @ (Ry @ Rx))
    return out


def affine_apply(pos, pos_ptr, M, t=None, index=None):
    """(R,3) float32: row r = M[b] (pos[v] - t[b]), v = index[r], b the mesh of v; out_i = (M_i0 d_0 + M_i1 d_1) + M_i2 d_2 in float32,
    every operation rounded on its own; NaN rows where v lies outside [0, V)"""
    pos, M = np.asarray(pos, dtype=np.float32), np.asarray(M, dtype=np.float32)
    V = pos.shape[0]
    v = np.arange(V) if index is None else np.asarray(index, dtype=np.int64)
    ok = (v >= 0) & (v < V)
    vv = np.where(ok, v, 0)
    b = np.searchsorted(np.asarray(pos_ptr)[1:], vv, side='right')
    d = pos[vv] if t is None else pos[vv] - np.asarray(t, dtype=np.float32)[b]
    Mb = M[b]
    out = np.empty((len(v), 3), dtype=np.float32)
    for i in range(3):
        out[:, i] = (Mb[:, i, 0] * d[:, 0] + Mb[:, i, 1] * d[:, 1]) + Mb[:, i, 2] * d[:, 2]
    out[~ok] = np.nan
    return out
