// Sparse transfer of per-sample features between two sample levels (pooling onto a coarser sample, unpooling back):
//
//   y[o, c] = sum_{e in [rowptr[o], rowptr[o+1])}  coef[e] * x[col[e], c]
//
// with coef[e] = weight[e] * phase[e] (or weight[e] * conj(phase[e])) for complex x -- the phase is the parallel transport into
// the receiving sample's frame -- and coef[e] = weight[e] for real x (scalar features).  The rows arrive as a CSR by OUTPUT row,
// so every output element is owned by one lane: no atomics, the terms of a row are added to a zero in ascending slot order, an
// empty row is written as zero, and two runs give the same bits.  The gradient to x is this kernel on the transposed CSR with the
// conjugate flag flipped (fieldconv_amd/transfer.py builds both CSRs once per plan).
//
// Work split.  A row of x is cut into UNITS of 8 bytes or more (one complex64, two float32 when C is even and the rows are
// 8-byte aligned, one float64, one complex128: a 16-byte load), U units per row, and the (row, unit) pairs are dealt to the lanes
// of the launch in row-major order: lane g owns unit g % U of row g / U.  With few channels a wavefront therefore holds several
// short rows (64 rows at U = 1; nobody idles on a one-slot unpool row), with U >= 64 a row has one or more wavefronts of its own,
// and in between (U = 48) no lane is left over, whatever C is.  The lanes of one row read one contiguous piece of each source
// row, and col / weight / phase of a slot are one address for all of them.  A lane walks its row's slots four at a time: four
// index and coefficient loads, then four independent row loads in flight, then the four multiply-adds in slot order.  A long
// pool row (a whole cell) is thus spread over U lanes that each do cell-size steps; the only serial chain is the one the fixed
// summation order asks for.  Lanes of different rows in one wavefront run as long as the longest of their rows.
//
// Nothing outside the buffers is touched whatever the index arrays hold: rowptr entries are clamped to [0, E] (and to the row's
// own start), and a slot whose col is outside [0, n_in) contributes nothing and reads nothing.
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"

namespace fc {

constexpr int kTransferThreads = 256;

template <typename T, int W> struct alignas(W * sizeof(T)) TransferUnit { T v[W]; };

// acc += coef * v for one unit: W scalars, complex as (re, im) pairs
template <typename T, bool CPLX, int W>
__device__ __forceinline__ void transfer_add(T (&acc)[W], T cr, T ci, const TransferUnit<T, W>& u) {
    if constexpr (CPLX) {
#pragma unroll
        for (int k = 0; k < W; k += 2) {
            acc[k] += cr * u.v[k] - ci * u.v[k + 1];
            acc[k + 1] += cr * u.v[k + 1] + ci * u.v[k];
        }
    } else {
#pragma unroll
        for (int k = 0; k < W; ++k) acc[k] += cr * u.v[k];
    }
}

// W: scalars per unit (2 per complex entry).  U: units per row, so a row holds U * W scalars.
template <typename T, bool CPLX, int W>
__global__ __launch_bounds__(kTransferThreads) void transfer_kernel(const T* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                                    const int32_t* __restrict__ col, const T* __restrict__ weight,
                                                                    const T* __restrict__ phase, int conj, int n_out, int n_in, int E,
                                                                    int U, T* __restrict__ y) {
    using Unit = TransferUnit<T, W>;
    const long long g = (long long)blockIdx.x * kTransferThreads + threadIdx.x;
    if (g >= (long long)n_out * U) return;
    const int row = (int)(g / U), unit = (int)(g - (long long)row * U);
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    const Unit* xu = reinterpret_cast<const Unit*>(x) + unit;
    const T sign = conj ? (T)-1 : (T)1;
    T acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = (T)0;

    auto coef = [&](int e, T& cr, T& ci) {
        const T w = weight[e];
        cr = w;
        ci = (T)0;
        if constexpr (CPLX) {
            if (phase) {
                cr = w * phase[2 * (size_t)e];
                ci = w * (sign * phase[2 * (size_t)e + 1]);
            }
        }
    };
    auto load = [&](int c) {
        Unit u;
        if ((unsigned)c < (unsigned)n_in) {
            u = xu[(size_t)c * U];
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) u.v[k] = (T)0;
        }
        return u;
    };

    int e = e0;
    for (; e + 4 <= e1; e += 4) {
        int c[4];
        T cr[4], ci[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            c[j] = col[e + j];
            coef(e + j, cr[j], ci[j]);
        }
        Unit u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = load(c[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) transfer_add<T, CPLX, W>(acc, cr[j], ci[j], u[j]);
    }
    for (; e < e1; ++e) {
        T cr, ci;
        coef(e, cr, ci);
        transfer_add<T, CPLX, W>(acc, cr, ci, load(col[e]));
    }
    Unit out;
#pragma unroll
    for (int k = 0; k < W; ++k) out.v[k] = acc[k];
    reinterpret_cast<Unit*>(y)[(size_t)row * U + unit] = out;
}

}  // namespace fc

namespace {

template <typename T, bool CPLX, int W>
int transfer_launch(const void* x, const int32_t* rowptr, const int32_t* col, const void* weight, const void* phase, int32_t conj,
                    int32_t n_out, int32_t n_in, int32_t E, int32_t U, void* y, hipStream_t s) {
    const long long lanes = (long long)n_out * U;
    const long long blocks = (lanes + fc::kTransferThreads - 1) / fc::kTransferThreads;
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::transfer_kernel<T, CPLX, W>), dim3((unsigned)blocks), dim3(fc::kTransferThreads), 0, s,
                       static_cast<const T*>(x), rowptr, col, static_cast<const T*>(weight), static_cast<const T*>(phase), (int)conj,
                       (int)n_out, (int)n_in, (int)E, (int)U, static_cast<T*>(y));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int fc_transfer(const void* x, const int32_t* rowptr, const int32_t* col, const void* weight, const void* phase, int32_t conj_phase,
                int32_t n_out, int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype, int32_t is_complex, void* y, void* stream) {
    if (n_out < 0 || n_in < 0 || n_slots < 0 || C < 1 || (dtype != FC_F32 && dtype != FC_F64) || (is_complex != 0 && is_complex != 1) ||
        (conj_phase != 0 && conj_phase != 1))
        return FC_ERR_BAD_ARGUMENT;
    if (n_out == 0) return FC_OK;
    if (!rowptr || !y || (n_slots > 0 && (!col || !weight || !x))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64)
        return is_complex ? transfer_launch<double, true, 2>(x, rowptr, col, weight, phase, conj_phase, n_out, n_in, n_slots, C, y, s)
                          : transfer_launch<double, false, 1>(x, rowptr, col, weight, nullptr, 0, n_out, n_in, n_slots, C, y, s);
    if (is_complex) return transfer_launch<float, true, 2>(x, rowptr, col, weight, phase, conj_phase, n_out, n_in, n_slots, C, y, s);
    const bool pairs = C % 2 == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 7) == 0;
    return pairs ? transfer_launch<float, false, 2>(x, rowptr, col, weight, nullptr, 0, n_out, n_in, n_slots, C / 2, y, s)
                 : transfer_launch<float, false, 1>(x, rowptr, col, weight, nullptr, 0, n_out, n_in, n_slots, C, y, s);
}

}  // extern "C"
