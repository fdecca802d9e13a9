// Intrinsic gradient of per-sample scalar features and its adjoint: the fixed (parameter-free) differential operator between real
// features and tangent-vector features.
//
//   coefficients   per query sample a, a weighted least-squares fit of a linear function over a's ball in a's own tangent plane.
//                  Slot e of row a holds the neighbour col[e] at log_a(col[e]) = m_e exp(i theta_e) in a's frame (logMag, logAng):
//                    p_e = m_e cosf(theta_e),  q_e = m_e sinf(theta_e),  omega_e = w[col[e]]  (1 without w)
//                    A11 = sum omega p p,  A12 = sum omega p q,  A22 = sum omega q q,  det = A11 A22 - A12 A12,  tr = A11 + A22
//                    valid[a] = det > rcond tr tr
//                    k_e = (omega_e / det) ((A22 p_e - A12 q_e) + i (A11 q_e - A12 p_e)),   diag[a] = sum_e k_e
//                  so that (G f)[a] = sum_e k_e (f[col[e]] - f[a]) is the fitted gradient as a complex number in a's frame: no
//                  transport is needed.  A slot is ACTIVE iff m_e > 0 and finite, theta_e finite, col[e] in [0, n), omega_e > 0 and
//                  finite; an inactive slot (the row [a, a], a zero-weight neighbour) takes no part in any sum, reads nothing out of
//                  range and has k_e = 0 exactly.  An invalid row (empty, one neighbour, collinear neighbours) has every k_e and
//                  diag exactly 0.
//   apply          y[a, c] = sum_e k_e (x[col[e], c] - x[a, c]),   x real, y complex
//   adjoint        gx[i, c] = so[i] ((sum_t Re(conj(k_t) si[col_t[t]] g[col_t[t], c])) - Re(conj(diag[i]) si[i] g[i, c])),  g complex, gx real,
//                  on the TRANSPOSED CSR; si / so are optional per-row scales (1 when absent), so that the divergence
//                  -W^-1 G^T W is one launch.
//
// Order of the sums.  Coefficients: one wavefront owns one row.  Lane l adds the terms of the active slots e0 + l, e0 + l + 64, ...
// of its row to a zero in ascending order; the 64 partial sums are then folded as p[l] += p[l + 32], p[l] += p[l + 16], ... ,
// p[0] += p[1] and lane 0's value is the sum.  The moments (A11, A12, A22) and diag (re, im) all use this order, which depends on
// the row's length alone; every operation is a float32 operation rounded on its own (no fused multiply-add), so apart from cosf and
// sinf -- the device library's -- numpy restates the bits.  apply / adjoint: fc_transfer.hip's work split.  A row is cut into units
// (two channels when C is even and the buffers are 8-byte aligned in float32, else one), the (row, unit) pairs are dealt to the
// lanes in row-major order -- the lanes across one source row are contiguous -- and a lane adds its row's terms to a zero in
// ascending slot order, four row loads in flight.  No atomics anywhere: two runs give the same bits.  A row without slots is
// written as zero; a constant x gives exactly zero, because every difference is.
//
// Nothing outside the buffers is touched whatever the index arrays hold: rowptr entries are clamped to [0, n_slots] and to the
// row's own start, and a slot whose col is outside [0, n) contributes nothing and reads nothing out of range (apply reads the row's
// own entry in its place: a zero difference).
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"

namespace fc {

constexpr int kDiffThreads = 256;

// ------------------------------------------------------------------ coefficients
struct DiffSlot {
    float p, q, omega;
    bool active;
};

__device__ __forceinline__ DiffSlot diff_slot(int e, const int32_t* __restrict__ col, const float* __restrict__ mag,
                                              const float* __restrict__ ang, const float* __restrict__ w, int n) {
#pragma clang fp contract(off)
    DiffSlot s;
    const int c = col[e];
    const float m = mag[e], th = ang[e];
    s.active = (unsigned)c < (unsigned)n && m > 0.f && isfinite(m) && isfinite(th);
    s.omega = 1.f;
    if (s.active && w) {
        s.omega = w[c];
        s.active = s.omega > 0.f && isfinite(s.omega);
    }
    s.p = s.active ? m * cosf(th) : 0.f;
    s.q = s.active ? m * sinf(th) : 0.f;
    return s;
}

// the 64 partial sums of a wavefront folded in the fixed order of the header; the same value in every lane
__device__ __forceinline__ float diff_fold(float v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return __shfl(v, 0, 64);
}

__device__ __forceinline__ void diff_moments(const DiffSlot& s, float& a11, float& a12, float& a22) {
#pragma clang fp contract(off)
    const float op = s.omega * s.p, oq = s.omega * s.q;
    const float t11 = op * s.p, t12 = op * s.q, t22 = oq * s.q;
    a11 = a11 + t11;
    a12 = a12 + t12;
    a22 = a22 + t22;
}

__device__ __forceinline__ bool diff_valid(float a11, float a12, float a22, float rcond, float& det) {
#pragma clang fp contract(off)
    const float x = a11 * a22, y = a12 * a12;
    det = x - y;
    const float tr = a11 + a22;
    const float bound = (rcond * tr) * tr;
    return det > bound;          // false for a NaN on either side
}

__device__ __forceinline__ float2 diff_coef(const DiffSlot& s, float a11, float a12, float a22, float det) {
#pragma clang fp contract(off)
    const float f = s.omega / det;
    const float u1 = a22 * s.p, u2 = a12 * s.q, v1 = a11 * s.q, v2 = a12 * s.p;
    const float re = u1 - u2, im = v1 - v2;
    return make_float2(f * re, f * im);
}

__global__ __launch_bounds__(kDiffThreads) void gradient_coefficients_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                             const float* __restrict__ mag, const float* __restrict__ ang,
                                                                             const float* __restrict__ w, float rcond, int n, int E,
                                                                             float2* __restrict__ coef, float2* __restrict__ diag,
                                                                             uint8_t* __restrict__ valid) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kWave - 1);
    const int row = blockIdx.x * (kDiffThreads / kWave) + (threadIdx.x >> 6);          // wave-uniform
    if (row >= n) return;
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    float a11 = 0.f, a12 = 0.f, a22 = 0.f;
    for (int e = e0 + lane; e < e1; e += kWave) {
        const DiffSlot s = diff_slot(e, col, mag, ang, w, n);
        if (s.active) diff_moments(s, a11, a12, a22);
    }
    a11 = diff_fold(a11);
    a12 = diff_fold(a12);
    a22 = diff_fold(a22);
    float det;
    const bool ok = diff_valid(a11, a12, a22, rcond, det);
    float dr = 0.f, di = 0.f;
    for (int e = e0 + lane; e < e1; e += kWave) {
        float2 k = make_float2(0.f, 0.f);
        if (ok) {
            const DiffSlot s = diff_slot(e, col, mag, ang, w, n);
            if (s.active) {
                k = diff_coef(s, a11, a12, a22, det);
                dr = dr + k.x;
                di = di + k.y;
            }
        }
        coef[e] = k;
    }
    dr = diff_fold(dr);
    di = diff_fold(di);
    if (lane == 0) {
        diag[row] = ok ? make_float2(dr, di) : make_float2(0.f, 0.f);
        valid[row] = ok ? 1 : 0;
    }
}

// ------------------------------------------------------------------ apply and adjoint
template <typename T, int W> struct alignas(W * sizeof(T)) DiffUnit { T v[W]; };

// y[row] = sum_e coef[e] * (x[col[e]] - x[row]): a lane owns W channels of a row, U units per row
template <typename T, int W>
__global__ __launch_bounds__(kDiffThreads) void gradient_apply_kernel(const T* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                                      const int32_t* __restrict__ col, const T* __restrict__ coef, int n, int E,
                                                                      int U, T* __restrict__ y) {
    using In = DiffUnit<T, W>;
    using Out = DiffUnit<T, 2>;
    const long long g = (long long)blockIdx.x * kDiffThreads + threadIdx.x;
    if (g >= (long long)n * U) return;
    const int row = (int)(g / U), unit = (int)(g - (long long)row * U);
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    const In* xu = reinterpret_cast<const In*>(x) + unit;
    T acc[2 * W];
#pragma unroll
    for (int k = 0; k < 2 * W; ++k) acc[k] = (T)0;
    In own = {};
    if (e1 > e0) own = xu[(size_t)row * U];

    // an out-of-range slot reads the row's own entry instead: its difference is zero, and nothing outside x is touched
    auto load = [&](int c) { return xu[(size_t)((unsigned)c < (unsigned)n ? c : row) * U]; };
    auto add = [&](T cr, T ci, const In& u) {
#pragma unroll
        for (int k = 0; k < W; ++k) {
            const T d = u.v[k] - own.v[k];
            acc[2 * k] += cr * d;
            acc[2 * k + 1] += ci * d;
        }
    };

    int e = e0;
    for (; e + 4 <= e1; e += 4) {
        int c[4];
        T cr[4], ci[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = col[e + j];
            cr[j] = coef[2 * (size_t)(e + j)];
            ci[j] = coef[2 * (size_t)(e + j) + 1];
        }
        In u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = load(c[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) add(cr[j], ci[j], u[j]);
    }
    for (; e < e1; ++e) add(coef[2 * (size_t)e], coef[2 * (size_t)e + 1], load(col[e]));
    Out* yu = reinterpret_cast<Out*>(y) + ((size_t)row * U + unit) * W;          // one complex entry per store
#pragma unroll
    for (int k = 0; k < W; ++k) {
        Out out;
        out.v[0] = acc[2 * k];
        out.v[1] = acc[2 * k + 1];
        yu[k] = out;
    }
}

// gx[row] = so[row] * (sum_t Re(conj(coef_t[t]) si[col_t[t]] g[col_t[t]]) - Re(conj(diag[row]) si[row] g[row])) on the transposed CSR
template <typename T, int W>
__global__ __launch_bounds__(kDiffThreads) void gradient_adjoint_kernel(const T* __restrict__ g, const int32_t* __restrict__ rowptr,
                                                                        const int32_t* __restrict__ col, const T* __restrict__ coef,
                                                                        const T* __restrict__ diag, const T* __restrict__ scale_in,
                                                                        const T* __restrict__ scale_out, int n, int E, int U,
                                                                        T* __restrict__ gx) {
    using In = DiffUnit<T, 2 * W>;
    using Out = DiffUnit<T, W>;
    const long long id = (long long)blockIdx.x * kDiffThreads + threadIdx.x;
    if (id >= (long long)n * U) return;
    const int row = (int)(id / U), unit = (int)(id - (long long)row * U);
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    const In* gu = reinterpret_cast<const In*>(g) + unit;
    T acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = (T)0;

    auto load = [&](int c, T& s) {
        In u;
        s = (T)1;
        if ((unsigned)c < (unsigned)n) {
            u = gu[(size_t)c * U];
            if (scale_in) s = scale_in[c];
        } else {
#pragma unroll
            for (int k = 0; k < 2 * W; ++k) u.v[k] = (T)0;
        }
        return u;
    };
    // Re(conj(k) s g) = kr (s gr) + ki (s gi)
    auto dot = [&](T cr, T ci, T s, const In& u, int k) { return cr * (s * u.v[2 * k]) + ci * (s * u.v[2 * k + 1]); };

    int e = e0;
    for (; e + 4 <= e1; e += 4) {
        int c[4];
        T cr[4], ci[4], s[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = col[e + j];
            cr[j] = coef[2 * (size_t)(e + j)];
            ci[j] = coef[2 * (size_t)(e + j) + 1];
        }
        In u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = load(c[j], s[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int k = 0; k < W; ++k) acc[k] += dot(cr[j], ci[j], s[j], u[j], k);
    }
    for (; e < e1; ++e) {
        T s;
        const In u = load(col[e], s);
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += dot(coef[2 * (size_t)e], coef[2 * (size_t)e + 1], s, u, k);
    }
    T s;
    const In u = load(row, s);
    const T dr = diag[2 * (size_t)row], di = diag[2 * (size_t)row + 1];
    const T so = scale_out ? scale_out[row] : (T)1;
    Out out;
#pragma unroll
    for (int k = 0; k < W; ++k) out.v[k] = so * (acc[k] - dot(dr, di, s, u, k));
    reinterpret_cast<Out*>(gx)[(size_t)row * U + unit] = out;
}

}  // namespace fc

namespace {

long long diff_blocks(int32_t n, int32_t U) { return ((long long)n * U + fc::kDiffThreads - 1) / fc::kDiffThreads; }

template <typename T, int W>
int apply_launch(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, int32_t n, int32_t E, int32_t U, void* y,
                 hipStream_t s) {
    const long long blocks = diff_blocks(n, U);
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::gradient_apply_kernel<T, W>), dim3((unsigned)blocks), dim3(fc::kDiffThreads), 0, s, static_cast<const T*>(x),
                       rowptr, col, static_cast<const T*>(coef), (int)n, (int)E, (int)U, static_cast<T*>(y));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, int W>
int adjoint_launch(const void* g, const int32_t* rowptr, const int32_t* col, const void* coef, const void* diag, const void* scale_in,
                   const void* scale_out, int32_t n, int32_t E, int32_t U, void* gx, hipStream_t s) {
    const long long blocks = diff_blocks(n, U);
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::gradient_adjoint_kernel<T, W>), dim3((unsigned)blocks), dim3(fc::kDiffThreads), 0, s, static_cast<const T*>(g),
                       rowptr, col, static_cast<const T*>(coef), static_cast<const T*>(diag), static_cast<const T*>(scale_in),
                       static_cast<const T*>(scale_out), (int)n, (int)E, (int)U, static_cast<T*>(gx));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

bool aligned8(const void* a, const void* b) { return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b)) & 7) == 0; }

}  // namespace

extern "C" {

int fc_gradient_coefficients(const int32_t* rowptr, const int32_t* col, const float* logMag, const float* logAng, const float* w, double rcond,
                             int32_t n, int32_t n_slots, void* coef, void* diag, uint8_t* valid, void* stream) {
    if (n < 0 || n_slots < 0 || !(rcond >= 0.0) || !(rcond <= 1.0)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!rowptr || !diag || !valid || (n_slots > 0 && (!col || !logMag || !logAng || !coef))) return FC_ERR_BAD_ARGUMENT;
    const int rows_per_block = fc::kDiffThreads / fc::kWave;
    const unsigned blocks = (unsigned)(((long long)n + rows_per_block - 1) / rows_per_block);
    hipLaunchKernelGGL(fc::gradient_coefficients_kernel, dim3(blocks), dim3(fc::kDiffThreads), 0, static_cast<hipStream_t>(stream), rowptr, col,
                       logMag, logAng, w, (float)rcond, (int)n, (int)n_slots, static_cast<float2*>(coef), static_cast<float2*>(diag), valid);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_gradient_apply(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, int32_t n, int32_t n_slots, int32_t C,
                      int32_t dtype, void* y, void* stream) {
    if (n < 0 || n_slots < 0 || C < 1 || (dtype != FC_F32 && dtype != FC_F64)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!rowptr || !y || (n_slots > 0 && (!col || !coef || !x))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64) return apply_launch<double, 1>(x, rowptr, col, coef, n, n_slots, C, y, s);
    return C % 2 == 0 && aligned8(x, y)
               ? apply_launch<float, 2>(x, rowptr, col, coef, n, n_slots, C / 2, y, s)
               : apply_launch<float, 1>(x, rowptr, col, coef, n, n_slots, C, y, s);
}

int fc_gradient_adjoint(const void* g, const int32_t* rowptr_t, const int32_t* col_t, const void* coef_t, const void* diag,
                        const void* scale_in, const void* scale_out, int32_t n, int32_t n_slots, int32_t C, int32_t dtype, void* gx,
                        void* stream) {
    if (n < 0 || n_slots < 0 || C < 1 || (dtype != FC_F32 && dtype != FC_F64)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!rowptr_t || !gx || !g || !diag || (n_slots > 0 && (!col_t || !coef_t))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64) return adjoint_launch<double, 1>(g, rowptr_t, col_t, coef_t, diag, scale_in, scale_out, n, n_slots, C, gx, s);
    return C % 2 == 0 && aligned8(gx, nullptr) && ((reinterpret_cast<uintptr_t>(g) & 15) == 0)
               ? adjoint_launch<float, 2>(g, rowptr_t, col_t, coef_t, diag, scale_in, scale_out, n, n_slots, C / 2, gx, s)
               : adjoint_launch<float, 1>(g, rowptr_t, col_t, coef_t, diag, scale_in, scale_out, n, n_slots, C, gx, s);
}

}  // extern "C"
