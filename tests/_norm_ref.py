"""numpy restatement of TangentNorm (fieldconv_amd.norm, csrc/fc_norm.hip): the definition and the two gradient formulas, in the
arithmetic of `real` (np.float32 or np.float64).

    W[b]    = sum_{n in b} w[n]
    m[b,c]  = sum_{n in b} w[n] |x[n,c]|^2 / W[b]          (0 where W[b] == 0, and for an empty mesh)
    r[b,c]  = 1 / sqrt(m[b,c] + eps)
    y[n,c]  = gain[c] r[b,c] x[n,c]
    t[b,c]  = sum_{n in b} re(x) re(gy) + im(x) im(gy)
    gx[n,c] = gain[c] r[b,c] gy[n,c] - gain[c] r[b,c]^3 t[b,c] (w[n] / W[b]) x[n,c]          (second term 0 where W[b] == 0)
    ggain[c] = sum_b r[b,c] t[b,c]

The sums over a mesh run in the order include/fieldconv_hip.h documents: chunks of 64 rows counted from the mesh's first row, four
running sums over the rows v, v + 4, ... of a chunk combined as (a_0 + a_1) + (a_2 + a_3), the chunks of a mesh the same way."""
import numpy as np

STANDARD_PTR = (0, 0, 1, 64, 129, 386)          # meshes of 0, 1, 63, 65 and 257 rows


def _four(parts, real):
    """parts (k,C) -> (C,): four running sums over the entries v, v + 4, ... in ascending order, (a_0 + a_1) + (a_2 + a_3)"""
    a = np.zeros((4,) + parts.shape[1:], dtype=real)
    for j in range(parts.shape[0]):
        a[j % 4] = a[j % 4] + parts[j]
    return (a[0] + a[1]) + (a[2] + a[3])


def mesh_sum(terms, real):
    """terms (n,C) of one mesh -> (C,)"""
    terms = terms.astype(real)
    chunks = [_four(terms[i:i + 64], real) for i in range(0, terms.shape[0], 64)]
    if not chunks:
        return np.zeros(terms.shape[1:], dtype=real)
    return _four(np.stack(chunks), real)


def _cast(x, w, gain, real):
    cdt = np.complex64 if real == np.float32 else np.complex128
    N, C = x.shape
    w = np.ones(N, dtype=real) if w is None else np.asarray(w).reshape(-1).astype(real)
    gain = np.ones(C, dtype=real) if gain is None else np.asarray(gain).reshape(-1).astype(real)
    return x.astype(cdt), w, gain, cdt


def statistics(x, ptr, w, eps, real):
    """(r (B,C), W (B,))"""
    x, w, _, _ = _cast(x, w, None, real)
    B, C = len(ptr) - 1, x.shape[1]
    r, W = np.zeros((B, C), dtype=real), np.zeros(B, dtype=real)
    for b in range(B):
        p0, p1 = ptr[b], ptr[b + 1]
        W[b] = mesh_sum(w[p0:p1, None], real)[0]
        s = mesh_sum(w[p0:p1, None] * (x.real[p0:p1] ** 2 + x.imag[p0:p1] ** 2), real)
        m = s / W[b] if W[b] > 0 else np.zeros(C, dtype=real)
        with np.errstate(divide='ignore'):          # eps = 0 and m = 0 (an empty mesh, a zero channel): inf, as on the device
            r[b] = real(1) / np.sqrt(m + real(eps))
    return r, W


def forward(x, ptr, w=None, gain=None, eps=1e-5, real=np.float64):
    """y (N,C) complex of `real`'s precision"""
    r, _ = statistics(x, ptr, w, eps, real)
    x, _, gain, cdt = _cast(x, w, gain, real)
    y = np.zeros(x.shape, dtype=cdt)
    for b in range(len(ptr) - 1):
        p0, p1 = ptr[b], ptr[b + 1]
        y[p0:p1] = ((gain * r[b])[None, :] * x[p0:p1]).astype(cdt)
    return y


def backward(x, gy, ptr, w=None, gain=None, eps=1e-5, real=np.float64):
    """(gx (N,C) complex, ggain (C,) real) for the cotangent gy (torch's convention for a real loss)"""
    r, W = statistics(x, ptr, w, eps, real)
    x, w, gain, cdt = _cast(x, w, gain, real)
    gy = gy.astype(cdt)
    gx, ggain = np.zeros(x.shape, dtype=cdt), np.zeros(x.shape[1], dtype=real)
    for b in range(len(ptr) - 1):
        p0, p1 = ptr[b], ptr[b + 1]
        t = mesh_sum(x.real[p0:p1] * gy.real[p0:p1] + x.imag[p0:p1] * gy.imag[p0:p1], real)
        a = gain * r[b]
        g = a[None, :] * gy[p0:p1]
        if W[b] > 0:
            g = g - ((a * r[b] * r[b] * t)[None, :] * (w[p0:p1] / W[b])[:, None]) * x[p0:p1]
        gx[p0:p1] = g.astype(cdt)
        ggain = ggain + r[b] * t
    return gx, ggain


def features(N, C, seed):
    """(N,C) complex128 with float32-representable parts of order 1"""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((N, C)).astype(np.float32) + 1j * rng.standard_normal((N, C)).astype(np.float32)).astype(np.complex128)


def weights(N, seed):
    """(N,) float64, float32-representable, in (0.1, 2.1): integration weights of an unevenly sampled surface"""
    return (0.1 + 2 * np.random.default_rng(seed).random(N)).astype(np.float32).astype(np.float64)


def gains(C, seed):
    return (0.5 + np.random.default_rng(seed).random(C)).astype(np.float32).astype(np.float64)


def loss(x, gy, ptr, w, gain, eps):
    """the real loss whose gradient at x (and gain) has the cotangent gy: sum re(conj(gy) y), in float64"""
    y = forward(x, ptr, w, gain, eps, np.float64)
    return float((gy.real * y.real + gy.imag * y.imag).sum())
