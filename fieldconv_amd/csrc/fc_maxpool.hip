// Max pooling by magnitude: over the rows of a transfer plan (fc_transfer_max, the max counterpart of fc_transfer.hip) and over the
// meshes of a batch (fc_segment_max_*, the max counterpart of fc_segment.hip).
//
//   key      of a complex entry z: k = fl(fl(re * re) + fl(im * im)) in z's scalar type, every operation rounded on its own (contraction
//            off: numpy gives the same bits).  |z| does not depend on the frame z is written in, so the choice is gauge invariant.
//            Of a real entry: k = x itself -- a plain max.
//   winner   among candidates (k, s), s the slot (transfer) or the row number (meshes): the largest k, ties to the smallest s.  A
//            candidate replaces the incumbent iff k_new > k_old, or k_new == k_old and s_new < s_old: a total order, so the result
//            does not depend on how the candidates are split over lanes, wavefronts or launches.  NaN is outside the contract: the
//            winner is then meaningless, but it is one of the candidates and nothing outside the buffers is touched.
//
// No atomics anywhere: every output element is owned by one lane, and two runs give the same bits.
//
// transfer   forward: fc_transfer.hip's work split -- a row of x is cut into units of 8 bytes or more (one complex64, two float32 when
//            C is even and the rows are 8-byte aligned, one float64, one complex128), lane g owns unit g % U of output row g / U and
//            walks the row's slots in ascending order, four row loads in flight, so "replace iff k_new > k_old" is the whole rule and a
//            row may be of any length.  A float32 pair keeps two independent winners.  The lane keeps the winning entry in registers;
//            only the winner's phase is read: y = u * x (complex), y = x bit for bit (real).  weight does not exist here.
//            backward: the same split on the transposed CSR.  slot[t] is the forward slot of transposed slot t; the lane of (input
//            row i, unit) walks i's slots in ascending order and adds conj(u[t]) * gy[out(t)] (real: gy[out(t)]) to a zero where
//            arg[out(t)] == slot[t].  gy and the phase are read for winners only.
// meshes     fc_segment.hpp's chunk-slot scheme: workgroup (chunk slot, channel tile) of 4 wavefronts x 64 lanes, lane = channel,
//            wavefront w takes the rows w, w + 4, ... of its 64-row chunk, the four are combined in the (k, s) order through LDS and
//            (key, row) goes to the partial buffers; a second launch (mesh, channel tile) combines the mesh's chunks the same way
//            and writes the value and the winning row.  The backward launch gives every (row, channel) its own thread.
//
// Nothing outside the buffers is touched whatever the index arrays hold: rowptr entries are clamped to [0, E] (and to the row's
// own start), a slot whose col is out of range is no candidate and reads nothing, arg / slot / index values are only compared,
// ptr entries are clamped to [0, N], and a partial row is checked before x is read at it.
#include "../../include/fieldconv_hip.h"
#include "fc_segment.hpp"

namespace fc {

constexpr int kMaxThreads = 256;

template <typename T> __device__ __forceinline__ T max_key(T re, T im) {
#pragma clang fp contract(off)          // (plain operators: __fmul_rn / __fadd_rn are header functions that hipcc contracts)
    const T a = re * re, b = im * im;
    return a + b;
}

// does the candidate (kn, sn) replace the incumbent (k, s)?  A negative s is "none".
template <typename T> __device__ __forceinline__ bool max_beats(T kn, int sn, T k, int s) {
    return sn >= 0 && (s < 0 || kn > k || (kn == k && sn < s));
}

__device__ __forceinline__ float max_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double max_sqrt(double v) { return sqrt(v); }

template <typename T, int W> struct alignas(W * sizeof(T)) MaxUnit { T v[W]; };
template <int NW> struct alignas(NW * sizeof(int32_t)) MaxArg { int32_t v[NW]; };

// ------------------------------------------------------------------------------------------------ over the rows of a plan
// W: scalars per unit (2 per complex entry), NW: winners per unit.  U: units per row.
template <typename T, bool CPLX, int W>
__global__ __launch_bounds__(kMaxThreads) void transfer_max_kernel(const T* __restrict__ x, const int32_t* __restrict__ rowptr,
                                                                   const int32_t* __restrict__ col, const T* __restrict__ phase, int conj,
                                                                   int n_out, int n_in, int E, int U, T* __restrict__ y,
                                                                   int32_t* __restrict__ arg) {
    constexpr int NW = CPLX ? W / 2 : W;
    using Unit = MaxUnit<T, W>;
    const long long g = (long long)blockIdx.x * kMaxThreads + threadIdx.x;
    if (g >= (long long)n_out * U) return;
    const int row = (int)(g / U), unit = (int)(g - (long long)row * U);
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    const Unit* xu = reinterpret_cast<const Unit*>(x) + unit;
    Unit best;
    T bk[NW];
    MaxArg<NW> bs;
#pragma unroll
    for (int k = 0; k < W; ++k) best.v[k] = (T)0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        bk[w] = (T)0;
        bs.v[w] = -1;
    }

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
    // slots arrive in ascending order: a later slot wins only with a strictly larger key
    auto take = [&](int e, int c, const Unit& u) {
        if ((unsigned)c >= (unsigned)n_in) return;
#pragma unroll
        for (int w = 0; w < NW; ++w) {
            T k;
            if constexpr (CPLX) k = max_key(u.v[2 * w], u.v[2 * w + 1]);
            else k = u.v[w];
            if (bs.v[w] < 0 || k > bk[w]) {
                bk[w] = k;
                bs.v[w] = e;
                if constexpr (CPLX) {
                    best.v[2 * w] = u.v[2 * w];
                    best.v[2 * w + 1] = u.v[2 * w + 1];
                } else {
                    best.v[w] = u.v[w];
                }
            }
        }
    };

    int e = e0;
    for (; e + 4 <= e1; e += 4) {
        int c[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) c[j] = col[e + j];
        Unit u[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = load(c[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) take(e + j, c[j], u[j]);
    }
    for (; e < e1; ++e) {
        const int c = col[e];
        take(e, c, load(c));
    }

    if constexpr (CPLX) {
        if (phase) {
            const T sign = conj ? (T)-1 : (T)1;
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (bs.v[w] >= 0) {
                    const T pr = phase[2 * (size_t)bs.v[w]], pi = sign * phase[2 * (size_t)bs.v[w] + 1];
                    const T xr = best.v[2 * w], xi = best.v[2 * w + 1];
                    best.v[2 * w] = pr * xr - pi * xi;
                    best.v[2 * w + 1] = pr * xi + pi * xr;
                }
        }
    }
    reinterpret_cast<Unit*>(y)[(size_t)row * U + unit] = best;
    reinterpret_cast<MaxArg<NW>*>(arg)[(size_t)row * U + unit] = bs;
}

// The transposed CSR: row i of it is input row i, col[t] the output row of slot t, slot[t] its slot number in the forward CSR.
template <typename T, bool CPLX, int W>
__global__ __launch_bounds__(kMaxThreads) void transfer_max_backward_kernel(const T* __restrict__ gy, const int32_t* __restrict__ arg,
                                                                            const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col,
                                                                            const int32_t* __restrict__ slot, const T* __restrict__ phase,
                                                                            int conj, int n_in, int n_out, int E, int U, T* __restrict__ gx) {
    constexpr int NW = CPLX ? W / 2 : W;
    using Unit = MaxUnit<T, W>;
    using Arg = MaxArg<NW>;
    const long long g = (long long)blockIdx.x * kMaxThreads + threadIdx.x;
    if (g >= (long long)n_in * U) return;
    const int row = (int)(g / U), unit = (int)(g - (long long)row * U);
    const int e0 = min(max(rowptr[row], 0), E), e1 = min(max(rowptr[row + 1], e0), E);
    const Unit* gu = reinterpret_cast<const Unit*>(gy) + unit;
    const Arg* au = reinterpret_cast<const Arg*>(arg) + unit;
    const T sign = conj ? (T)1 : (T)-1;          // conj(u): the imaginary part of u = phase or conj(phase), negated
    T acc[W];
#pragma unroll
    for (int k = 0; k < W; ++k) acc[k] = (T)0;

    auto winners = [&](int o) {
        Arg a;
        if ((unsigned)o < (unsigned)n_out) {
            a = au[(size_t)o * U];
        } else {
#pragma unroll
            for (int w = 0; w < NW; ++w) a.v[w] = -1;
        }
        return a;
    };
    auto add = [&](int t, int o, int f, const Arg& a) {
        if ((unsigned)o >= (unsigned)n_out || f < 0) return;
        bool any = false;
#pragma unroll
        for (int w = 0; w < NW; ++w) any = any || a.v[w] == f;
        if (!any) return;
        const Unit v = gu[(size_t)o * U];
        if constexpr (CPLX) {
            T pr = (T)1, pi = (T)0;
            if (phase) {
                pr = phase[2 * (size_t)t];
                pi = sign * phase[2 * (size_t)t + 1];
            }
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (a.v[w] == f) {
                    acc[2 * w] += pr * v.v[2 * w] - pi * v.v[2 * w + 1];
                    acc[2 * w + 1] += pr * v.v[2 * w + 1] + pi * v.v[2 * w];
                }
        } else {
#pragma unroll
            for (int w = 0; w < NW; ++w)
                if (a.v[w] == f) acc[w] += v.v[w];
        }
    };

    int t = e0;
    for (; t + 4 <= e1; t += 4) {
        int o[4], f[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            o[j] = col[t + j];
            f[j] = slot[t + j];
        }
        Arg a[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) a[j] = winners(o[j]);
#pragma unroll
        for (int j = 0; j < 4; ++j) add(t + j, o[j], f[j], a[j]);
    }
    for (; t < e1; ++t) {
        const int o = col[t];
        add(t, o, slot[t], winners(o));
    }
    Unit out;
#pragma unroll
    for (int k = 0; k < W; ++k) out.v[k] = acc[k];
    reinterpret_cast<Unit*>(gx)[(size_t)row * U + unit] = out;
}

// ------------------------------------------------------------------------------------------------ over the meshes of a batch
// reference utils/field.py:10-16: both components strictly inside (-1e-7, 1e-7), whatever the dtype
template <typename T> __device__ __forceinline__ bool max_origin(SegCx<T> z) {
    const T e = (T)1e-7;
    return z.x < e && z.x > -e && z.y < e && z.y > -e;
}

template <typename T, bool CPLX> __device__ __forceinline__ T max_key_at(const void* __restrict__ x, size_t idx) {
    if constexpr (CPLX) {
        const SegCx<T> z = static_cast<const SegCx<T>*>(x)[idx];
        return max_key(z.x, z.y);
    } else {
        return static_cast<const T*>(x)[idx];
    }
}

// the four wavefronts' candidates of this lane in the (k, s) order; the result is valid in wavefront 0
template <typename T> __device__ __forceinline__ void max_combine(T (*sk)[64], int (*ss)[64], T& k, int& s, int wave, int lane) {
    sk[wave][lane] = k;
    ss[wave][lane] = s;
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int w = 1; w < kSegWaves; ++w)
            if (max_beats(sk[w][lane], ss[w][lane], k, s)) {
                k = sk[w][lane];
                s = ss[w][lane];
            }
    }
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(kSegThreads) void segment_max_partial_kernel(const void* __restrict__ x, const int64_t* __restrict__ ptr, int B,
                                                                          int N, int C, T* __restrict__ pkey, int32_t* __restrict__ prow) {
    __shared__ T sk[kSegWaves][64];
    __shared__ int ss[kSegWaves][64];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const int b = seg_mesh_of_slot(ptr, B, N, g);
    int p0, p1, r0, r1;
    seg_range(ptr, b, N, p0, p1);
    if (!seg_chunk_rows(g, b, p0, p1, r0, r1)) return;       // a spare slot (the whole workgroup leaves)
    T k = (T)0;
    int s = -1;
    if (c < C)
        for (int r = r0 + wave; r < r1; r += kSegWaves) {     // ascending rows: a later row wins only with a strictly larger key
            const T kn = max_key_at<T, CPLX>(x, (size_t)r * C + c);
            if (s < 0 || kn > k) {
                k = kn;
                s = r;
            }
        }
    max_combine(sk, ss, k, s, wave, lane);
    if (wave == 0 && c < C) {
        pkey[(size_t)g * C + c] = k;
        prow[(size_t)g * C + c] = s;
    }
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(kSegThreads) void segment_max_finish_kernel(const void* __restrict__ x, const T* __restrict__ pkey,
                                                                         const int32_t* __restrict__ prow, const int64_t* __restrict__ ptr,
                                                                         int N, int C, T* __restrict__ out, int32_t* __restrict__ index) {
    __shared__ T sk[kSegWaves][64];
    __shared__ int ss[kSegWaves][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    int p0, p1;
    seg_range(ptr, b, N, p0, p1);
    const int n = p1 - p0, chunks = (n + kSegRows - 1) / kSegRows, base = p0 / kSegRows + b;
    T k = (T)0;
    int s = -1;
    if (c < C)
        for (int j = wave; j < chunks; j += kSegWaves) {
            const T kn = pkey[(size_t)(base + j) * C + c];
            const int sn = prow[(size_t)(base + j) * C + c];
            if (max_beats(kn, sn, k, s)) {
                k = kn;
                s = sn;
            }
        }
    max_combine(sk, ss, k, s, wave, lane);
    if (wave == 0 && c < C) {
        T v = (T)0;
        if (s >= 0 && s < N) {
            if constexpr (CPLX) {
                const SegCx<T> z = static_cast<const SegCx<T>*>(x)[(size_t)s * C + c];
                v = max_origin(z) ? (T)0 : max_sqrt(k);
            } else {
                v = k;                                          // the key of a real entry is the entry, bit for bit
            }
        } else {
            s = -1;
        }
        out[(size_t)b * C + c] = v;
        index[(size_t)b * C + c] = s;
    }
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(kSegThreads) void segment_max_backward_kernel(const void* __restrict__ x, const T* __restrict__ g,
                                                                           const int32_t* __restrict__ index, const int64_t* __restrict__ ptr,
                                                                           int B, int N, int C, void* __restrict__ gx) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    if (c >= C) return;
    const int rend = (int)min((long long)N, ((long long)blockIdx.x + 1) * kSegRows);
    int b = 0, p0 = 0, p1 = 0;
    bool have = false;
    for (int r = blockIdx.x * kSegRows + wave; r < rend; r += kSegWaves) {
        if (!have || r >= p1) {                              // rows ascend: look the mesh up again only past the current one's end
            b = seg_mesh_of_row(ptr, B, N, r);
            seg_range(ptr, b, N, p0, p1);
            have = true;
        }
        const bool won = r >= p0 && r < p1 && index[(size_t)b * C + c] == r;
        const T s = won ? g[(size_t)b * C + c] : (T)0;
        const size_t idx = (size_t)r * C + c;
        if constexpr (CPLX) {
            SegCx<T> o;
            o.x = (T)0;
            o.y = (T)0;
            if (won) {
                const SegCx<T> z = static_cast<const SegCx<T>*>(x)[idx];
                if (!max_origin(z)) {
                    const T q = s / max_sqrt(z.x * z.x + z.y * z.y);
                    o.x = z.x * q;
                    o.y = z.y * q;
                }
            }
            static_cast<SegCx<T>*>(gx)[idx] = o;
        } else {
            static_cast<T*>(gx)[idx] = s;
        }
    }
}

}  // namespace fc

namespace {

bool aligned8(const void* a, const void* b, const void* c) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 7) == 0;
}

template <typename T, bool CPLX, int W>
int transfer_max_launch(const void* x, const int32_t* rowptr, const int32_t* col, const void* phase, int32_t conj, int32_t n_out,
                        int32_t n_in, int32_t E, int32_t U, void* y, int32_t* arg, hipStream_t s) {
    const long long blocks = ((long long)n_out * U + fc::kMaxThreads - 1) / fc::kMaxThreads;
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::transfer_max_kernel<T, CPLX, W>), dim3((unsigned)blocks), dim3(fc::kMaxThreads), 0, s, static_cast<const T*>(x),
                       rowptr, col, static_cast<const T*>(phase), (int)conj, (int)n_out, (int)n_in, (int)E, (int)U, static_cast<T*>(y), arg);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, bool CPLX, int W>
int transfer_max_backward_launch(const void* gy, const int32_t* arg, const int32_t* rowptr, const int32_t* col, const int32_t* slot,
                                 const void* phase, int32_t conj, int32_t n_out, int32_t n_in, int32_t E, int32_t U, void* gx, hipStream_t s) {
    const long long blocks = ((long long)n_in * U + fc::kMaxThreads - 1) / fc::kMaxThreads;
    if (blocks > 2147483647LL) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL((fc::transfer_max_backward_kernel<T, CPLX, W>), dim3((unsigned)blocks), dim3(fc::kMaxThreads), 0, s,
                       static_cast<const T*>(gy), arg, rowptr, col, slot, static_cast<const T*>(phase), (int)conj, (int)n_in, (int)n_out, (int)E,
                       (int)U, static_cast<T*>(gx));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

bool transfer_max_dims_ok(int32_t n_out, int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype, int32_t is_complex, int32_t conj_phase) {
    return n_out >= 0 && n_in >= 0 && n_slots >= 0 && C >= 1 && (dtype == FC_F32 || dtype == FC_F64) && (is_complex == 0 || is_complex == 1) &&
           (conj_phase == 0 || conj_phase == 1);
}

bool segment_max_dims_ok(int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t is_complex) {
    return fc::seg_shape_ok(N, B, C) && (dtype == FC_F32 || dtype == FC_F64) && (is_complex == 0 || is_complex == 1);
}

template <typename T, bool CPLX>
int segment_max_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, void* out, int32_t* index, void* pkey,
                        int32_t* prow, hipStream_t s) {
    const dim3 block(fc::kSegThreads);
    const unsigned tiles = (unsigned)((C + 63) / 64);
    hipLaunchKernelGGL((fc::segment_max_partial_kernel<T, CPLX>), dim3((unsigned)fc::seg_slots(N, B), tiles), block, 0, s, x, ptr, B, N, C,
                       static_cast<T*>(pkey), prow);
    hipLaunchKernelGGL((fc::segment_max_finish_kernel<T, CPLX>), dim3((unsigned)B, tiles), block, 0, s, x, static_cast<const T*>(pkey), prow,
                       ptr, N, C, static_cast<T*>(out), index);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, bool CPLX>
int segment_max_backward(const void* x, const void* g, const int32_t* index, const int64_t* ptr, int32_t N, int32_t B, int32_t C, void* gx,
                         hipStream_t s) {
    if (N == 0) return FC_OK;
    const unsigned tiles = (unsigned)((C + 63) / 64);
    hipLaunchKernelGGL((fc::segment_max_backward_kernel<T, CPLX>), dim3((unsigned)((N + fc::kSegRows - 1) / fc::kSegRows), tiles),
                       dim3(fc::kSegThreads), 0, s, x, static_cast<const T*>(g), index, ptr, B, N, C, gx);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int fc_transfer_max(const void* x, const int32_t* rowptr, const int32_t* col, const void* phase, int32_t conj_phase, int32_t n_out,
                    int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype, int32_t is_complex, void* y, int32_t* arg, void* stream) {
    if (!transfer_max_dims_ok(n_out, n_in, n_slots, C, dtype, is_complex, conj_phase)) return FC_ERR_BAD_ARGUMENT;
    if (n_out == 0) return FC_OK;
    if (!rowptr || !y || !arg || (n_slots > 0 && (!col || !x))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64)
        return is_complex ? transfer_max_launch<double, true, 2>(x, rowptr, col, phase, conj_phase, n_out, n_in, n_slots, C, y, arg, s)
                          : transfer_max_launch<double, false, 1>(x, rowptr, col, nullptr, 0, n_out, n_in, n_slots, C, y, arg, s);
    if (is_complex) return transfer_max_launch<float, true, 2>(x, rowptr, col, phase, conj_phase, n_out, n_in, n_slots, C, y, arg, s);
    return C % 2 == 0 && aligned8(x, y, arg) ? transfer_max_launch<float, false, 2>(x, rowptr, col, nullptr, 0, n_out, n_in, n_slots, C / 2, y, arg, s)
                                             : transfer_max_launch<float, false, 1>(x, rowptr, col, nullptr, 0, n_out, n_in, n_slots, C, y, arg, s);
}

int fc_transfer_max_backward(const void* grad_y, const int32_t* arg, const int32_t* rowptr_t, const int32_t* col_t, const int32_t* slot_t,
                             const void* phase_t, int32_t conj_phase, int32_t n_out, int32_t n_in, int32_t n_slots, int32_t C, int32_t dtype,
                             int32_t is_complex, void* grad_x, void* stream) {
    if (!transfer_max_dims_ok(n_out, n_in, n_slots, C, dtype, is_complex, conj_phase)) return FC_ERR_BAD_ARGUMENT;
    if (n_in == 0) return FC_OK;
    if (!rowptr_t || !grad_x || (n_slots > 0 && (!col_t || !slot_t || !grad_y || !arg))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F64)
        return is_complex ? transfer_max_backward_launch<double, true, 2>(grad_y, arg, rowptr_t, col_t, slot_t, phase_t, conj_phase, n_out, n_in,
                                                                          n_slots, C, grad_x, s)
                          : transfer_max_backward_launch<double, false, 1>(grad_y, arg, rowptr_t, col_t, slot_t, nullptr, 0, n_out, n_in,
                                                                           n_slots, C, grad_x, s);
    if (is_complex)
        return transfer_max_backward_launch<float, true, 2>(grad_y, arg, rowptr_t, col_t, slot_t, phase_t, conj_phase, n_out, n_in, n_slots, C,
                                                            grad_x, s);
    return C % 2 == 0 && aligned8(grad_y, grad_x, arg)
               ? transfer_max_backward_launch<float, false, 2>(grad_y, arg, rowptr_t, col_t, slot_t, nullptr, 0, n_out, n_in, n_slots, C / 2, grad_x, s)
               : transfer_max_backward_launch<float, false, 1>(grad_y, arg, rowptr_t, col_t, slot_t, nullptr, 0, n_out, n_in, n_slots, C, grad_x, s);
}

int fc_segment_max_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t is_complex, void* out,
                           int32_t* index, void* partial_key, int32_t* partial_row, void* stream) {
    if (!segment_max_dims_ok(N, B, C, dtype, is_complex) || !ptr || !out || !index || !partial_key || !partial_row || (N > 0 && !x))
        return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F32)
        return is_complex ? segment_max_forward<float, true>(x, ptr, N, B, C, out, index, partial_key, partial_row, s)
                          : segment_max_forward<float, false>(x, ptr, N, B, C, out, index, partial_key, partial_row, s);
    return is_complex ? segment_max_forward<double, true>(x, ptr, N, B, C, out, index, partial_key, partial_row, s)
                      : segment_max_forward<double, false>(x, ptr, N, B, C, out, index, partial_key, partial_row, s);
}

int fc_segment_max_backward(const void* x, const void* grad_out, const int32_t* index, const int64_t* ptr, int32_t N, int32_t B, int32_t C,
                            int32_t dtype, int32_t is_complex, void* grad_x, void* stream) {
    if (!segment_max_dims_ok(N, B, C, dtype, is_complex) || !ptr || !grad_out || !index || (N > 0 && (!grad_x || (is_complex && !x))))
        return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F32)
        return is_complex ? segment_max_backward<float, true>(x, grad_out, index, ptr, N, B, C, grad_x, s)
                          : segment_max_backward<float, false>(nullptr, grad_out, index, ptr, N, B, C, grad_x, s);
    return is_complex ? segment_max_backward<double, true>(x, grad_out, index, ptr, N, B, C, grad_x, s)
                      : segment_max_backward<double, false>(nullptr, grad_out, index, ptr, N, B, C, grad_x, s);
}

}  // extern "C"
