// Heat diffusion of per-sample features: the connection Laplacian of the support graph and the solve y = (W + t S)^-1 W x by a fixed
// number of Jacobi-preconditioned conjugate-gradient steps, one diffusion time per channel.
//
//   coefficients   The stiffness matrix S = 1/2 D^H C D, (D v)[e] = v[b] - u_e v[a] for a row e = [a, b] of supp_edges with transport
//                  u_e = xp[e], as a merged CSR: row i holds one entry per row [i, b] (col b, -1/2 c_e conj(u_e); the OUT entries, in
//                  ascending e) and then one per row [a, i] (col a, -1/2 c_e u_e; the IN entries, in ascending e).  The host lays the
//                  pattern out (edge[k] = e, or -e - 1 for an out entry); the kernel fills the values:
//                    active  e  iff a != b, m_e = logMag[e] > 0 and finite, xp[e] finite, w_a and w_b > 0 and finite (1 without w)
//                    c_e = ((w_a * w_b) * expf(-((m_e * m_e) / four_h))) / norm      four_h = fl32(4 h), norm = fl32(4 pi h^2)
//                    g_e = -0.5 * c_e      coef = (g_e Re u, -/+ g_e Im u)      creal = g_e      (all exactly 0 on an inactive row)
//                    diag[i]      = 0.5 * (sum over the row's entries, in entry order, of c_e |u_e|^2 (out) or c_e (in))
//                    diag_real[i] = 0.5 * (the same sum of c_e): the matrix of real features, u = 1
//                  every operation a float32 operation rounded on its own; expf is the device library's.  One thread per row.
//   apply          y[i, c] = so[i] * ((sum over the row's entries of coef_e * (si[col_e] x[col_e, c])) + diag[i] * (si[i] x[i, c])),
//                  the entry sum added to a zero in entry order; si / so optional row scales.  so = -1 / w: the Laplacian -W^-1 S;
//                  si = -1 / w: its adjoint -S W^-1 (S is Hermitian: no transposed CSR).  One lane per (row, channel).
//   solve          per mesh and channel, `iters` steps of preconditioned CG on (W + t_c S) y = rhs (include/fieldconv_hip.h states the
//                  recurrence).  One workgroup of 1024 threads owns one mesh and one UNIT of channels -- 16 bytes of a row: 4 float32,
//                  2 float64 or complex64, 1 complex128 channel -- through all iterations: thread l owns the rows l, l + 1024, ... of
//                  the mesh, keeps their y, r and q in a workspace slot only it touches, and is the only writer of their search
//                  direction p.  p is the one vector gathered at neighbours: it lives in LDS while the mesh fits (kDfLdsRows rows of
//                  16 bytes), else in a fourth workspace slot; the loop is the same.  The two inner products are double: a lane adds
//                  the terms of its rows in ascending order to a zero, the 64 lanes of a wavefront are folded v[l] += v[l + 32],
//                  v[l + 16], ..., v[l + 1], and the 16 wavefronts' sums are added in index order.  No operation is contracted, so
//                  the bits of a channel depend on its mesh's own rows and entries alone: not on C, on the unit it shares, on where p
//                  lives, or on the other meshes of a batch.  No atomics, no grid-wide wait: every loop is bounded by iters and the
//                  mesh's size, every barrier is the workgroup's own and is reached by all of its threads.
//
// Nothing outside the buffers is touched whatever the index arrays hold: rowptr entries are clamped to [0, n_entries] and to the row's
// own start, mesh ranges to [0, n], and an entry whose col lies outside its row's mesh (apply: outside [0, n)) contributes nothing and
// reads nothing.
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_geodesic_relax.hpp"
#include "fc_workspace.hpp"

namespace fc {

constexpr int kDfThreads = 1024;
constexpr int kDfWaves = kDfThreads / kWave;
constexpr int kDfLdsRows = 10000;                            // 160 000 B of p beside the reduction scratch, of the CU's 163 840
constexpr int kDfScratchBytes = kDfWaves * 4 * 8;            // one double per wavefront and channel of a unit (at most 4)
constexpr int kDfApplyThreads = 256;

// ------------------------------------------------------------------ coefficients
__global__ __launch_bounds__(kDfApplyThreads) void diffusion_coefficients_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ edge, const float* __restrict__ mag,
    const float2* __restrict__ xp, const float* __restrict__ w, float four_h, float norm, int n, int n_edges, int n_entries,
    float2* __restrict__ coef, float* __restrict__ creal, float* __restrict__ diag, float* __restrict__ diag_real) {
#pragma clang fp contract(off)
    const int i = blockIdx.x * kDfApplyThreads + threadIdx.x;
    if (i >= n) return;
    const int k0 = min(max(rowptr[i], 0), n_entries), k1 = min(max(rowptr[i + 1], k0), n_entries);
    float d = 0.f, dr = 0.f;
    for (int k = k0; k < k1; ++k) {
        const int code = edge[k], j = col[k];
        const bool out = code < 0;
        const int e = out ? -(code + 1) : code;
        float2 c = make_float2(0.f, 0.f);
        float g = 0.f;
        if ((unsigned)e < (unsigned)n_edges && (unsigned)j < (unsigned)n && j != i) {
            const float m = mag[e];
            const float2 u = xp[e];
            const float wi = w ? w[i] : 1.f, wj = w ? w[j] : 1.f;
            if (m > 0.f && isfinite(m) && isfinite(u.x) && isfinite(u.y) && wi > 0.f && isfinite(wi) && wj > 0.f && isfinite(wj)) {
                const float m2 = m * m;
                const float q = m2 / four_h;
                const float ww = out ? wi * wj : wj * wi;          // (w_a * w_b: a is this row for an out entry)
                const float ce = (ww * expf(-q)) / norm;
                g = -0.5f * ce;
                const float gi = g * u.y;
                c = make_float2(g * u.x, out ? -gi : gi);
                float term = ce;
                if (out) {
                    const float a2 = u.x * u.x, b2 = u.y * u.y;
                    term = ce * (a2 + b2);
                }
                d = d + term;
                dr = dr + ce;
            }
        }
        coef[k] = c;
        creal[k] = g;
    }
    diag[i] = 0.5f * d;
    diag_real[i] = 0.5f * dr;
}

// ------------------------------------------------------------------ the matrix row, shared by apply and solve
// K scalars of one row: CB = K channels (real) or K / 2 (complex)
template <typename T, int K> struct alignas(K * sizeof(T)) DfUnit { T v[K]; };

// acc += coef * u for one entry: complex (cr, ci) or real (cr)
template <typename T, int K, bool kComplex>
__device__ __forceinline__ void df_mac(DfUnit<T, K>& acc, T cr, T ci, const DfUnit<T, K>& u) {
#pragma clang fp contract(off)
    if constexpr (kComplex) {
#pragma unroll
        for (int k = 0; k < K; k += 2) {
            const T a = cr * u.v[k], b = ci * u.v[k + 1], c = cr * u.v[k + 1], d = ci * u.v[k];
            const T re = a - b, im = c + d;
            acc.v[k] = acc.v[k] + re;
            acc.v[k + 1] = acc.v[k + 1] + im;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T a = cr * u.v[k];
            acc.v[k] = acc.v[k] + a;
        }
    }
}

// ------------------------------------------------------------------ apply
template <typename T, bool kComplex>
__global__ __launch_bounds__(kDfApplyThreads) void diffusion_apply_kernel(const T* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                                          const int32_t* __restrict__ col, const T* __restrict__ coef,
                                                                          const T* __restrict__ diag, const T* __restrict__ scale_in,
                                                                          const T* __restrict__ scale_out, int n, int n_entries, int C,
                                                                          T* __restrict__ y) {
#pragma clang fp contract(off)
    constexpr int K = kComplex ? 2 : 1;
    using U = DfUnit<T, K>;
    const long long g = (long long)blockIdx.x * kDfApplyThreads + threadIdx.x;
    if (g >= (long long)n * C) return;
    const int row = (int)(g / C), ch = (int)(g - (long long)row * C);
    const int k0 = min(max(rowptr[row], 0), n_entries), k1 = min(max(rowptr[row + 1], k0), n_entries);
    const U* xu = reinterpret_cast<const U*>(x) + ch;
    auto load = [&](int r) {
        U u = xu[(size_t)r * C];
        if (scale_in) {
            const T s = scale_in[r];
#pragma unroll
            for (int k = 0; k < K; ++k) u.v[k] = s * u.v[k];
        }
        return u;
    };
    U acc;
#pragma unroll
    for (int k = 0; k < K; ++k) acc.v[k] = (T)0;
    for (int e = k0; e < k1; ++e) {
        const int c = col[e];
        if ((unsigned)c >= (unsigned)n) continue;
        const T cr = kComplex ? coef[2 * (size_t)e] : coef[e], ci = kComplex ? coef[2 * (size_t)e + 1] : (T)0;
        df_mac<T, K, kComplex>(acc, cr, ci, load(c));
    }
    const U own = load(row);
    const T d = diag[row], so = scale_out ? scale_out[row] : (T)1;
    U out;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const T dx = d * own.v[k];
        const T s = acc.v[k] + dx;
        out.v[k] = so * s;
    }
    reinterpret_cast<U*>(y)[(size_t)row * C + ch] = out;
}

// ------------------------------------------------------------------ solve
struct df_args {
    const void* x;              // (n, C) right-hand side
    const void* t;              // (C) diffusion times, x's scalar type
    const void* w;              // (n) x's scalar type, or null for 1
    const void* diag;           // (n) x's scalar type
    const int32_t* rowptr;      // (n + 1)
    const int32_t* col;         // (n_entries)
    const void* coef;           // (n_entries) complex or real, x's scalar type
    const int64_t* ptr;         // (B + 1) mesh ranges, or null: one mesh, all n rows
    void* y;                    // (n, C)
    void* lam;                  // null, or (n, C): the unscaled solution in mode 1
    void* resid;                // null, or (B, C) x's scalar type: sqrt(rz) at exit
    void* ws;                   // the state slots
    int32_t n, n_entries, C, B, iters, mode;
    int32_t max_rows;           // no mesh is taken to be larger (the caller's bound: what the LDS and the grid were sized for)
};

// the sum of one double per thread over the workgroup in the fixed order of the header, the same value in every thread;
// scratch: kDfWaves * 4 doubles of LDS; NV values at once
template <int NV>
__device__ __forceinline__ void df_block_sum(double (&v)[NV], double* scratch) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) v[k] = v[k] + __shfl_down(v[k], off, 64);
        if (lane == 0) scratch[wave * 4 + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NV; ++k) {
        double s = 0.0;
        for (int i = 0; i < kDfWaves; ++i) s = s + scratch[i * 4 + k];
        v[k] = s;
    }
    __syncthreads();
}

template <typename T, bool kComplex, bool kLds>
__global__ __launch_bounds__(kDfThreads) void diffusion_solve_kernel(const df_args a) {
#pragma clang fp contract(off)
    constexpr int K = 16 / (int)sizeof(T);               // scalars of a unit
    constexpr int S = kComplex ? 2 : 1;                  // scalars of a channel
    constexpr int CB = K / S;                            // channels of a unit
    constexpr int V = kLds ? 3 : 4;                      // workspace slots of a unit: y, r, q (, p)
    using U = DfUnit<T, K>;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* const scratch = reinterpret_cast<double*>(smem);
    const int units = (a.C + CB - 1) / CB;
    const int mesh = blockIdx.x / units, unit = blockIdx.x - mesh * units;
    const int tid = threadIdx.x;
    int r0 = 0, nb = a.n;
    if (a.ptr) {
        r0 = (int)gf_clamp(a.ptr[mesh], 0, a.n);
        nb = (int)gf_clamp(a.ptr[mesh + 1], r0, a.n) - r0;
    }
    nb = min(nb, a.max_rows);
    const int c0 = unit * CB;
    const T* const x = static_cast<const T*>(a.x);
    const T* const w = static_cast<const T*>(a.w);
    const T* const diag = static_cast<const T*>(a.diag);
    const T* const coef = static_cast<const T*>(a.coef);
    U* const slot = static_cast<U*>(a.ws) + (size_t)unit * V * (size_t)a.n + r0;          // slot v of this mesh: slot + v * n
    U* const ys = slot;
    U* const rs = slot + (size_t)a.n;
    U* const qs = slot + 2 * (size_t)a.n;
    U* const p = kLds ? reinterpret_cast<U*>(smem + kDfScratchBytes) : slot + 3 * (size_t)a.n;

    T tc[CB];
    bool bad[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) {
        tc[k] = c0 + k < a.C ? static_cast<const T*>(a.t)[c0 + k] : (T)0;
        bad[k] = !(tc[k] >= (T)0) || !isfinite(tc[k]);
    }

    // q = (W + t S) p of one row, from the gathered p
    auto matvec = [&](int i, const U& own) {
        const int row = r0 + i;
        const int k0 = min(max(a.rowptr[row], 0), a.n_entries), k1 = min(max(a.rowptr[row + 1], k0), a.n_entries);
        U acc;
#pragma unroll
        for (int k = 0; k < K; ++k) acc.v[k] = (T)0;
        for (int e = k0; e < k1; ++e) {
            const int c = a.col[e] - r0;
            if ((unsigned)c >= (unsigned)nb) continue;
            const T cr = kComplex ? coef[2 * (size_t)e] : coef[e], ci = kComplex ? coef[2 * (size_t)e + 1] : (T)0;
            df_mac<T, K, kComplex>(acc, cr, ci, p[c]);
        }
        const T d = diag[row], wi = w ? w[row] : (T)1;
        U q;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T dx = d * own.v[k];
            const T sx = acc.v[k] + dx;
            const T wx = wi * own.v[k], ts = tc[k / S] * sx;
            q.v[k] = wx + ts;
        }
        return q;
    };
    // z = r / P, P = w + t d where that is positive, else 0
    auto precondition = [&](int i, const U& r) {
        const int row = r0 + i;
        const T d = diag[row], wi = w ? w[row] : (T)1;
        U z;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const T td = tc[k / S] * d;
            const T P = wi + td;
            z.v[k] = P > (T)0 ? r.v[k] / P : (T)0;
        }
        return z;
    };
    auto dot = [&](const U& u, const U& v, double (&s)[CB]) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const double pr = (double)u.v[k] * (double)v.v[k];
            s[k / S] = s[k / S] + pr;
        }
    };

    // start: y0 (mode 0: x; mode 1: x / w, 0 where w is not positive) goes to p's place to be gathered once
    for (int i = tid; i < nb; i += kDfThreads) {
        U y0;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = c0 + k / S;
            y0.v[k] = c < a.C ? x[((size_t)(r0 + i) * a.C + c) * S + k % S] : (T)0;
        }
        U rhs = y0;
        const T wi = w ? w[r0 + i] : (T)1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (a.mode == 0) rhs.v[k] = wi * y0.v[k];
            else y0.v[k] = wi > (T)0 ? y0.v[k] / wi : (T)0;
        }
        ys[i] = y0;
        rs[i] = rhs;
        p[i] = y0;
    }
    __syncthreads();
    double rz[CB];
#pragma unroll
    for (int k = 0; k < CB; ++k) rz[k] = 0.0;
    for (int i = tid; i < nb; i += kDfThreads) {
        const U q = matvec(i, p[i]);
        U r = rs[i];
#pragma unroll
        for (int k = 0; k < K; ++k) r.v[k] = r.v[k] - q.v[k];
        const U z = precondition(i, r);
        rs[i] = r;
        qs[i] = z;          // (z0 waits in q's slot until every thread has gathered y0)
        dot(r, z, rz);
    }
    df_block_sum<CB>(rz, scratch);
    for (int i = tid; i < nb; i += kDfThreads) p[i] = qs[i];
    __syncthreads();

    for (int it = 0; it < a.iters; ++it) {
        double pq[CB];
#pragma unroll
        for (int k = 0; k < CB; ++k) pq[k] = 0.0;
        for (int i = tid; i < nb; i += kDfThreads) {
            const U own = p[i];
            const U q = matvec(i, own);
            qs[i] = q;
            dot(own, q, pq);
        }
        df_block_sum<CB>(pq, scratch);
        T alpha[CB];
#pragma unroll
        for (int k = 0; k < CB; ++k) alpha[k] = (T)(pq[k] > 0.0 ? rz[k] / pq[k] : 0.0);
        double rz_new[CB];
#pragma unroll
        for (int k = 0; k < CB; ++k) rz_new[k] = 0.0;
        for (int i = tid; i < nb; i += kDfThreads) {
            const U own = p[i], q = qs[i];
            U y = ys[i], r = rs[i];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const T al = alpha[k / S];
                if (al != (T)0) {
                    const T ap = al * own.v[k], aq = al * q.v[k];
                    y.v[k] = y.v[k] + ap;
                    r.v[k] = r.v[k] - aq;
                }
            }
            ys[i] = y;
            rs[i] = r;
            const U z = precondition(i, r);
            dot(r, z, rz_new);
        }
        df_block_sum<CB>(rz_new, scratch);          // (its barriers: every gather of p is over before p changes)
        T beta[CB];
#pragma unroll
        for (int k = 0; k < CB; ++k) {
            beta[k] = (T)(rz[k] > 0.0 ? rz_new[k] / rz[k] : 0.0);
            rz[k] = rz_new[k];
        }
        for (int i = tid; i < nb; i += kDfThreads) {
            const U z = precondition(i, rs[i]);
            U own = p[i];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const T bp = beta[k / S] * own.v[k];
                own.v[k] = z.v[k] + bp;
            }
            p[i] = own;
        }
        __syncthreads();
    }

    const T nan = (T)__int_as_float(0x7fc00000);
    for (int i = tid; i < nb; i += kDfThreads) {
        const U y = ys[i];
        const T wi = w ? w[r0 + i] : (T)1;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int c = c0 + k / S;
            if (c >= a.C) continue;
            const size_t at = ((size_t)(r0 + i) * a.C + c) * S + k % S;
            const T v = bad[k / S] ? nan : y.v[k];
            static_cast<T*>(a.y)[at] = a.mode == 0 || bad[k / S] ? v : wi * v;
            if (a.lam) static_cast<T*>(a.lam)[at] = v;
        }
    }
    if (a.resid && tid == 0) {
#pragma unroll
        for (int k = 0; k < CB; ++k)
            if (c0 + k < a.C) static_cast<T*>(a.resid)[(size_t)mesh * a.C + c0 + k] = bad[k] ? nan : (T)sqrt(rz[k]);
    }
}

// ------------------------------------------------------------------ gt: the two fixed-order reductions
// part[b, c] = sum over the rows i of mesh b of Re(conj(lam[i, c]) sy[i, c]) in double: thread (j, l) of 16 x 64 adds the rows
// j, j + 16, ... of channel 64 g + l in ascending order, then the 16 partial sums are added in index order
template <typename T, bool kComplex>
__global__ __launch_bounds__(kDfThreads) void diffusion_dot_kernel(const T* __restrict__ lam, const T* __restrict__ sy,
                                                                   const int64_t* __restrict__ ptr, int n, int C, int groups,
                                                                   double* __restrict__ part) {
#pragma clang fp contract(off)
    constexpr int S = kComplex ? 2 : 1;
    __shared__ double fold[kDfWaves][kWave];
    const int mesh = blockIdx.x / groups, group = blockIdx.x - mesh * groups;
    const int l = threadIdx.x & (kWave - 1), j = threadIdx.x >> 6;
    const int c = group * kWave + l;
    int r0 = 0, r1 = n;
    if (ptr) {
        r0 = (int)gf_clamp(ptr[mesh], 0, n);
        r1 = (int)gf_clamp(ptr[mesh + 1], r0, n);
    }
    double s = 0.0;
    if (c < C)
        for (int i = r0 + j; i < r1; i += kDfWaves) {
            const size_t at = ((size_t)i * C + c) * S;
#pragma unroll
            for (int k = 0; k < S; ++k) {
                const double pr = (double)lam[at + k] * (double)sy[at + k];
                s = s + pr;
            }
        }
    fold[j][l] = s;
    __syncthreads();
    if (j == 0 && c < C) {
        double total = 0.0;
        for (int k = 0; k < kDfWaves; ++k) total = total + fold[k][l];
        part[(size_t)mesh * C + c] = total;
    }
}

// gt[c] = -(part[0, c] + part[1, c] + ...), rounded once to T
template <typename T>
__global__ void diffusion_gt_kernel(const double* __restrict__ part, int B, int C, T* __restrict__ gt) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    double s = 0.0;
    for (int b = 0; b < B; ++b) s = s + part[(size_t)b * C + c];
    gt[c] = (T)(-s);
}

}  // namespace fc

namespace {

using fc::Carver;

int df_units(int32_t C, int32_t dtype, int32_t is_complex) {
    const int cb = (dtype == FC_F64 ? 2 : 4) / (is_complex ? 2 : 1);
    return (C + cb - 1) / cb;
}

bool df_in_lds(int32_t max_rows, int32_t where) { return where == 0 && max_rows <= fc::kDfLdsRows; }

struct DfWorkspace { void* state; double* part; };
DfWorkspace df_layout(Carver& c, int32_t n, int32_t B, int32_t C, int32_t dtype, int32_t is_complex, bool lds) {
    DfWorkspace l;
    l.state = c.take<void>((size_t)df_units(C, dtype, is_complex) * (lds ? 3 : 4) * (size_t)n * 16);
    l.part = c.take<double>((size_t)B * (size_t)C * sizeof(double));
    return l;
}

template <typename T, bool kComplex>
int solve_launch(fc::df_args a, int32_t max_rows, bool lds, hipStream_t s) {
    static bool lds_ok[fc::kMaxDevices] = {};
    const unsigned grid = (unsigned)a.B * (unsigned)df_units(a.C, sizeof(T) == 8 ? FC_F64 : FC_F32, kComplex);
    if (lds) {
        const size_t bytes = fc::kDfScratchBytes + 16 * (size_t)max_rows;
        if (bytes > 64 * 1024) {
            const int st = fc::gf_allow_lds(reinterpret_cast<const void*>(fc::diffusion_solve_kernel<T, kComplex, true>), lds_ok,
                                            fc::kDfScratchBytes + 16 * (size_t)fc::kDfLdsRows);
            if (st != FC_OK) return st;
        }
        hipLaunchKernelGGL((fc::diffusion_solve_kernel<T, kComplex, true>), dim3(grid), dim3(fc::kDfThreads), bytes, s, a);
    } else {
        hipLaunchKernelGGL((fc::diffusion_solve_kernel<T, kComplex, false>), dim3(grid), dim3(fc::kDfThreads), (size_t)fc::kDfScratchBytes, s,
                           a);
    }
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, bool kComplex>
int apply_launch(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, const void* diag, const void* si, const void* so,
                 int32_t n, int32_t n_entries, int32_t C, void* y, hipStream_t s) {
    const long long blocks = ((long long)n * C + fc::kDfApplyThreads - 1) / fc::kDfApplyThreads;
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::diffusion_apply_kernel<T, kComplex>), dim3((unsigned)blocks), dim3(fc::kDfApplyThreads), 0, s,
                       static_cast<const T*>(x), rowptr, col, static_cast<const T*>(coef), static_cast<const T*>(diag), static_cast<const T*>(si),
                       static_cast<const T*>(so), (int)n, (int)n_entries, (int)C, static_cast<T*>(y));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, bool kComplex>
int dot_launch(const void* lam, const void* sy, const int64_t* ptr, int32_t n, int32_t B, int32_t C, double* part, void* gt, hipStream_t s) {
    const int groups = (C + fc::kWave - 1) / fc::kWave;
    hipLaunchKernelGGL((fc::diffusion_dot_kernel<T, kComplex>), dim3((unsigned)B * groups), dim3(fc::kDfThreads), 0, s, static_cast<const T*>(lam),
                       static_cast<const T*>(sy), ptr, (int)n, (int)C, groups, part);
    hipLaunchKernelGGL((fc::diffusion_gt_kernel<T>), dim3((unsigned)groups), dim3(fc::kWave), 0, s, part, (int)B, (int)C, static_cast<T*>(gt));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

bool df_dtype_ok(int32_t dtype, int32_t is_complex) { return (dtype == FC_F32 || dtype == FC_F64) && (is_complex == 0 || is_complex == 1); }

}  // namespace

extern "C" {

int32_t fc_diffusion_lds_rows(void) { return fc::kDfLdsRows; }

int fc_diffusion_coefficients(const int32_t* rowptr, const int32_t* col, const int32_t* edge, const float* logMag, const void* xp,
                              const float* w, double h, int32_t n, int32_t n_edges, int32_t n_entries, void* coef, float* coef_real,
                              float* diag, float* diag_real, void* stream) {
    if (n < 0 || n_edges < 0 || n_entries < 0 || !(h > 0.0) || !(h < 1e30)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!rowptr || !diag || !diag_real || (n_entries > 0 && (!col || !edge || !logMag || !xp || !coef || !coef_real))) return FC_ERR_BAD_ARGUMENT;
    const float four_h = (float)(4.0 * h), norm = (float)(4.0 * 3.14159265358979323846 * h * h);
    if (!(four_h > 0.f) || !(norm > 0.f)) return FC_ERR_BAD_ARGUMENT;
    const unsigned blocks = (unsigned)(((long long)n + fc::kDfApplyThreads - 1) / fc::kDfApplyThreads);
    hipLaunchKernelGGL(fc::diffusion_coefficients_kernel, dim3(blocks), dim3(fc::kDfApplyThreads), 0, static_cast<hipStream_t>(stream), rowptr,
                       col, edge, logMag, static_cast<const float2*>(xp), w, four_h, norm, (int)n, (int)n_edges, (int)n_entries,
                       static_cast<float2*>(coef), coef_real, diag, diag_real);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_diffusion_apply(const void* x, const int32_t* rowptr, const int32_t* col, const void* coef, const void* diag, const void* scale_in,
                       const void* scale_out, int32_t n, int32_t n_entries, int32_t C, int32_t dtype, int32_t is_complex, void* y,
                       void* stream) {
    if (n < 0 || n_entries < 0 || C < 1 || !df_dtype_ok(dtype, is_complex)) return FC_ERR_BAD_ARGUMENT;
    if (n == 0) return FC_OK;
    if (!rowptr || !x || !y || !diag || (n_entries > 0 && (!col || !coef))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64)
        return is_complex ? apply_launch<double, true>(x, rowptr, col, coef, diag, scale_in, scale_out, n, n_entries, C, y, s)
                          : apply_launch<double, false>(x, rowptr, col, coef, diag, scale_in, scale_out, n, n_entries, C, y, s);
    return is_complex ? apply_launch<float, true>(x, rowptr, col, coef, diag, scale_in, scale_out, n, n_entries, C, y, s)
                      : apply_launch<float, false>(x, rowptr, col, coef, diag, scale_in, scale_out, n, n_entries, C, y, s);
}

size_t fc_diffusion_workspace_bytes(int32_t n, int32_t B, int32_t C, int32_t dtype, int32_t is_complex, int32_t max_rows, int32_t where) {
    if (n < 0 || B < 1 || C < 1 || !df_dtype_ok(dtype, is_complex)) return 0;
    return fc::carved_bytes(df_layout, n, B, C, dtype, is_complex, df_in_lds(max_rows, where));
}

int fc_diffusion_solve(const void* x, const void* t, const void* w, const void* diag, const int32_t* rowptr, const int32_t* col,
                       const void* coef, const int64_t* ptr, int32_t n, int32_t n_entries, int32_t B, int32_t C, int32_t max_rows,
                       int32_t dtype, int32_t is_complex, int32_t iters, int32_t mode, int32_t where, void* y, void* lam, void* resid,
                       void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || n_entries < 0 || B < 1 || C < 1 || !df_dtype_ok(dtype, is_complex) || iters < 1 || iters > 1024 || (mode != 0 && mode != 1) ||
        (where != 0 && where != 1) || max_rows < 0 || max_rows > n || (!ptr && (B != 1 || max_rows != n)))
        return FC_ERR_BAD_ARGUMENT;
    if ((long long)B * df_units(C, dtype, is_complex) > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    if (!t || !rowptr || !diag || (n > 0 && (!x || !y)) || (n_entries > 0 && (!col || !coef))) return FC_ERR_BAD_ARGUMENT;
    const bool lds = df_in_lds(max_rows, where);
    Carver carver(workspace);
    const DfWorkspace l = df_layout(carver, n, B, C, dtype, is_complex, lds);
    if (!fc::gf_workspace_ok(carver.used, workspace, workspace_bytes)) return FC_ERR_WORKSPACE;
    fc::df_args a = {x, t, w, diag, rowptr, col, coef, ptr, y, lam, resid, l.state, n, n_entries, C, B, iters, mode, max_rows};
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64) return is_complex ? solve_launch<double, true>(a, max_rows, lds, s) : solve_launch<double, false>(a, max_rows, lds, s);
    return is_complex ? solve_launch<float, true>(a, max_rows, lds, s) : solve_launch<float, false>(a, max_rows, lds, s);
}

int fc_diffusion_time_gradient(const void* lam, const void* sy, const int64_t* ptr, int32_t n, int32_t B, int32_t C, int32_t dtype,
                               int32_t is_complex, void* gt, void* workspace, size_t workspace_bytes, void* stream) {
    if (n < 0 || B < 1 || C < 1 || !df_dtype_ok(dtype, is_complex) || !gt || (n > 0 && (!lam || !sy)) || (!ptr && B != 1)) return FC_ERR_BAD_ARGUMENT;
    if ((long long)B * ((C + fc::kWave - 1) / fc::kWave) > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    const size_t need = fc::align256((size_t)B * (size_t)C * sizeof(double));
    if (!workspace || workspace_bytes < need) return FC_ERR_WORKSPACE;
    double* part = static_cast<double*>(workspace);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64)
        return is_complex ? dot_launch<double, true>(lam, sy, ptr, n, B, C, part, gt, s) : dot_launch<double, false>(lam, sy, ptr, n, B, C, part, gt, s);
    return is_complex ? dot_launch<float, true>(lam, sy, ptr, n, B, C, part, gt, s) : dot_launch<float, false>(lam, sy, ptr, n, B, C, part, gt, s);
}

}  // extern "C"
