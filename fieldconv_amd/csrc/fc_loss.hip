// Losses of the reference's nn package on the device (TwinLoss, TwinEval, LabelSmoothingLoss) and the pair kernels under them:
//   fc_pair_sqdist                  d2 of every pair of a list;
//   fc_twin_loss_forward/_backward  the twin loss over positive and negative pair lists, and its gradients by a per-row sum of the
//                                   pairs that touch the row (store-and-sum: no float atomics, bitwise reproducible);
//   fc_twin_count_dense             #{(a,b) : d2 < thr} and #{d2 > thr} over ALL N_T x N_S pairs, no pair list;
//   fc_label_smoothing_forward/_backward.
// One pair distance for all of them: d2(a,b) = ((t0*t0 + t1*t1) + t2*t2) + ... with t_c = xT[a,c] - xS[b,c], c ascending, every
// operation rounded on its own (no contraction), so that the kernels agree bit for bit and numpy restates them exactly.
// Sums over pairs / rows that end in one scalar run in double in a fixed order (wavefront, then workgroup, then one workgroup over
// the per-workgroup partials in index order): two runs give the same bits.
#include "../../include/fieldconv_hip.h"
#include "fc_pair.hpp"          // d2_step / pair_d2 and the dense tile: shared with fc_match.hip
#include "fc_workspace.hpp"

namespace fc {

constexpr int kLossThreads = 1024;          // workgroup of the kernels that end in a scalar: one pair / row (group) per thread
constexpr int kLossWaves = kLossThreads / 64;
constexpr int kGradThreads = 256;
constexpr int kDenseMaxThr = 16;
constexpr int kDenseMaxGrid = 2048;

// out = sum(partials[2g]) / den0 + sum(partials[2g+1]) / den1 over g < G.  One workgroup: thread t takes g = t, t + 1024, ...
template <typename T>
__global__ __launch_bounds__(kLossThreads) void final_sum_kernel(const double* __restrict__ partials, int G, double den0, double den1,
                                                                 T* __restrict__ out) {
    __shared__ double slots[kLossWaves];
    double s0 = 0, s1 = 0;
    for (int g = threadIdx.x; g < G; g += kLossThreads) {
        s0 += partials[2 * (size_t)g];
        s1 += partials[2 * (size_t)g + 1];
    }
    s0 = block_sum<kLossWaves>(s0, slots);
    s1 = block_sum<kLossWaves>(s1, slots);
    if (threadIdx.x == 0) out[0] = static_cast<T>(s0 / den0 + s1 / den1);
}

template <typename T>
__global__ __launch_bounds__(256) void pair_sqdist_kernel(const T* __restrict__ xS, const T* __restrict__ xT,
                                                          const int64_t* __restrict__ pairs, int64_t K, int C, T* __restrict__ d2) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= K) return;
    d2[k] = pair_d2(xT + (size_t)pairs[2 * k] * C, xS + (size_t)pairs[2 * k + 1] * C, C);
}

// relu(h) as torch has it (a NaN stays a NaN)
template <typename T>
__device__ __forceinline__ T relu_keep_nan(T h) {
    return h > 0 ? h : (h != h ? h : static_cast<T>(0));
}

// Pair k < P is p_[k], pair k >= P is n_[k - P].  yN is float32 whatever T is, and 1 - yN is rounded in float32 (as the reference's
// module, which draws float32 weights, has it).  A pair with an index outside its feature matrix reads nothing and counts as NaN.
template <typename T>
__global__ __launch_bounds__(kLossThreads) void twin_forward_kernel(const T* __restrict__ xS, int nS, const T* __restrict__ xT, int nT, int C,
                                                                    const int64_t* __restrict__ p_, int64_t P,
                                                                    const int64_t* __restrict__ n_, int64_t M, const float* __restrict__ yN,
                                                                    T mu, T* __restrict__ d2, double* __restrict__ partials,
                                                                    T* __restrict__ loss) {
    __shared__ double slots[kLossWaves];
    const int64_t k = (int64_t)blockIdx.x * kLossThreads + threadIdx.x;
    double sp = 0, sn = 0;
    if (k < P + M) {
        const int64_t* pr = k < P ? p_ + 2 * k : n_ + 2 * (k - P);
        const int64_t a = pr[0], b = pr[1];
        const bool in = a >= 0 && a < nT && b >= 0 && b < nS;
        const T d = in ? pair_d2(xT + (size_t)a * C, xS + (size_t)b * C, C) : quiet_nan<T>();
        d2[k] = d;
        if (k < P) {
            sp = (double)d;
        } else {
            const T y = static_cast<T>(yN[k - P]), rest = static_cast<T>(1.0f - yN[k - P]);
            sn = (double)(y * d + rest * relu_keep_nan(mu - d));
        }
    }
    sp = block_sum<kLossWaves>(sp, slots);
    sn = block_sum<kLossWaves>(sn, slots);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            loss[0] = static_cast<T>(sp / (double)P + sn / (double)M);
        } else {
            partials[2 * (size_t)blockIdx.x] = sp;
            partials[2 * (size_t)blockIdx.x + 1] = sn;
        }
    }
}

// G lanes per feature row; rows [0, nT) are xT's, rows [nT, nT + nS) are xS's.  rowptr / order: the pairs (numbered as in the forward
// kernel) that touch each row, in list order (a stable sort of the pair list by row).  Each lane sums its channels over the row's
// pairs in that order and stores; rows that no pair touches store zeros.
template <typename T, int G>
__global__ __launch_bounds__(kGradThreads) void twin_backward_kernel(const T* __restrict__ xS, int nS, const T* __restrict__ xT, int nT, int C,
                                                                     const int64_t* __restrict__ p_, int64_t P,
                                                                     const int64_t* __restrict__ n_, int64_t M,
                                                                     const float* __restrict__ yN, T mu, const T* __restrict__ d2,
                                                                     const T* __restrict__ g, const int64_t* __restrict__ rowptrT,
                                                                     const int64_t* __restrict__ orderT,
                                                                     const int64_t* __restrict__ rowptrS,
                                                                     const int64_t* __restrict__ orderS, T* __restrict__ gT,
                                                                     T* __restrict__ gS) {
    const int64_t row = (int64_t)blockIdx.x * (kGradThreads / G) + threadIdx.x / G;
    const int l = threadIdx.x % G;
    if (row >= (int64_t)nT + nS) return;
    const bool tside = row < nT;
    const int64_t r = tside ? row : row - nT;
    const int64_t* rowptr = tside ? rowptrT : rowptrS;
    const int64_t* order = tside ? orderT : orderS;
    T* grad = tside ? gT : gS;
    const int64_t lo = rowptr[r], hi = rowptr[r + 1];
    const T two_g = static_cast<T>(2) * g[0];
    const T cp = two_g / static_cast<T>(P);
    for (int c = l; c < C; c += G) {
        T acc = 0;
        for (int64_t s = lo; s < hi; ++s) {
            const int64_t k = order[s];
            const int64_t* pr = k < P ? p_ + 2 * k : n_ + 2 * (k - P);
            const int64_t a = pr[0], b = pr[1];
            T coef = cp;
            if (k >= P) {
                const T y = static_cast<T>(yN[k - P]), rest = static_cast<T>(1.0f - yN[k - P]);
                const T step = (mu - d2[k] > 0) ? static_cast<T>(1) : static_cast<T>(0);
                coef = two_g * (y - rest * step) / static_cast<T>(M);
            }
            const bool in = a >= 0 && a < nT && b >= 0 && b < nS;
            const T t = in ? xT[(size_t)a * C + c] - xS[(size_t)b * C + c] : quiet_nan<T>();
            acc += tside ? coef * t : -(coef * t);
        }
        grad[(size_t)r * C + c] = acc;
    }
}

template <typename T>
struct DenseThresholds {
    T v[kDenseMaxThr];
};

// Tiles of 64 xT rows x 64 xS rows, kDenseChunk channels at a time through LDS (transposed: [channel][row]); lane (ty, tx) owns
// rows 4*ty..4*ty+3 of xT and 4*tx..4*tx+3 of xS.  counts[t] += #{d2 < thr[t]}, counts[NT_total + t] += #{d2 > thr[t]} (thresholds
// beyond the caller's are +inf copies whose counters are not written back).
template <typename T, int NT>
__global__ __launch_bounds__(kDenseThreads) void twin_count_dense_kernel(const T* __restrict__ xS, int nS, const T* __restrict__ xT, int nT,
                                                                         int C, DenseThresholds<T> thr, int n_thr, int64_t tilesS,
                                                                         int64_t tiles, unsigned long long* __restrict__ counts) {
    __shared__ __attribute__((aligned(16))) T sT[kDenseChunk][kDensePitch];
    __shared__ __attribute__((aligned(16))) T sS[kDenseChunk][kDensePitch];
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    int below[NT], above[NT];
#pragma unroll
    for (int t = 0; t < NT; ++t) below[t] = above[t] = 0;
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int a0 = (int)(tile / tilesS) * kDenseTile, b0 = (int)(tile % tilesS) * kDenseTile;
        T acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = 0;
        for (int c0 = 0; c0 < C; c0 += kDenseChunk) {
            const int nc = min(kDenseChunk, C - c0);
            __syncthreads();
#pragma unroll
            for (int e = tid; e < kDenseTile * kDenseChunk; e += kDenseThreads) {
                const int row = e / kDenseChunk, ch = e % kDenseChunk;
                const bool cin = ch < nc;
                sT[ch][row] = (cin && a0 + row < nT) ? xT[(size_t)(a0 + row) * C + c0 + ch] : static_cast<T>(0);
                sS[ch][row] = (cin && b0 + row < nS) ? xS[(size_t)(b0 + row) * C + c0 + ch] : static_cast<T>(0);
            }
            __syncthreads();
            auto channel = [&](int c) {
                T a[4], b[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[i] = sT[c][4 * ty + i];
                    b[i] = sS[c][4 * tx + i];
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[i][j] = d2_step(acc[i][j], a[i], b[j]);
            };
            if (nc == kDenseChunk) {
#pragma unroll
                for (int c = 0; c < kDenseChunk; ++c) channel(c);
            } else {
                for (int c = 0; c < nc; ++c) channel(c);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                // a pair outside the matrices compares false both ways
                const T d = (a0 + 4 * ty + i < nT && b0 + 4 * tx + j < nS) ? acc[i][j] : quiet_nan<T>();
#pragma unroll
                for (int t = 0; t < NT; ++t) {
                    below[t] += d < thr.v[t] ? 1 : 0;
                    above[t] += d > thr.v[t] ? 1 : 0;
                }
            }
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        int lo = below[t], hi = above[t];
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            lo += __shfl_xor(lo, m, 64);
            hi += __shfl_xor(hi, m, 64);
        }
        if ((tid & 63) == 0 && t < n_thr) {
            if (lo) atomicAdd(counts + t, (unsigned long long)lo);
            if (hi) atomicAdd(counts + n_thr + t, (unsigned long long)hi);
        }
    }
}

template <typename T>
__device__ __forceinline__ T t_exp(T x);
template <>
__device__ __forceinline__ float t_exp<float>(float x) { return expf(x); }
template <>
__device__ __forceinline__ double t_exp<double>(double x) { return exp(x); }
template <typename T>
__device__ __forceinline__ T t_log(T x);
template <>
__device__ __forceinline__ float t_log<float>(float x) { return logf(x); }
template <>
__device__ __forceinline__ double t_log<double>(double x) { return log(x); }

template <typename T, int G>
__device__ __forceinline__ T group_sum(T v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <typename T, int G>
__device__ __forceinline__ T group_max(T v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// Row statistics with G lanes per row (lane l takes classes l, l + G, ...): the row maximum, sum_k exp(x_k - max) and
// sum_k t_k w_k, t_k = conf at the target and off elsewhere.  The same in every lane of the group.
template <typename T, int G>
__device__ __forceinline__ void ls_row_stats(const T* __restrict__ x, int K, int64_t target, const T* __restrict__ w, T conf, T off,
                                             int l, T& mx, T& se, T& stw, T& stwx) {
    mx = -INFINITY;
    for (int k = l; k < K; k += G) mx = fmax(mx, x[k]);
    mx = group_max<T, G>(mx);
    se = 0, stw = 0, stwx = 0;
    for (int k = l; k < K; k += G) {
        const T v = x[k];
        const T tw = (k == target ? conf : off) * (w ? w[k] : static_cast<T>(1));
        se += t_exp<T>(v - mx);
        stw += tw;
        stwx += tw * (v - mx);
    }
    se = group_sum<T, G>(se);
    stw = group_sum<T, G>(stw);
    stwx = group_sum<T, G>(stwx);
}

// loss_n = -sum_k t_k w_k (x_k - lse) = log(se) * sum(t w) - sum(t w (x - max))
template <typename T, int G>
__global__ __launch_bounds__(kLossThreads) void label_smoothing_forward_kernel(const T* __restrict__ pred, const int64_t* __restrict__ target,
                                                                               const T* __restrict__ weight, int64_t N, int K, T conf,
                                                                               T off, double* __restrict__ partials,
                                                                               T* __restrict__ loss) {
    __shared__ double slots[kLossWaves];
    const int64_t n = (int64_t)blockIdx.x * (kLossThreads / G) + threadIdx.x / G;
    const int l = threadIdx.x % G;
    double v = 0;
    if (n < N) {
        T mx, se, stw, stwx;
        ls_row_stats<T, G>(pred + (size_t)n * K, K, target[n], weight, conf, off, l, mx, se, stw, stwx);
        if (l == 0) v = (double)(t_log<T>(se) * stw - stwx);
    }
    v = block_sum<kLossWaves>(v, slots);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) {
            loss[0] = static_cast<T>(v / (double)N);
        } else {
            partials[2 * (size_t)blockIdx.x] = v;
            partials[2 * (size_t)blockIdx.x + 1] = 0;
        }
    }
}

// g_nj = (g / N) (softmax_nj sum_k t_nk w_k - t_nj w_j), the softmax recomputed from pred
template <typename T, int G>
__global__ __launch_bounds__(kLossThreads) void label_smoothing_backward_kernel(const T* __restrict__ pred, const int64_t* __restrict__ target,
                                                                                const T* __restrict__ weight, const T* __restrict__ g,
                                                                                int64_t N, int K, T conf, T off, T* __restrict__ gpred) {
    const int64_t n = (int64_t)blockIdx.x * (kLossThreads / G) + threadIdx.x / G;
    const int l = threadIdx.x % G;
    if (n >= N) return;          // (whole groups leave together: G divides 64)
    const T* x = pred + (size_t)n * K;
    const int64_t tg = target[n];
    T mx, se, stw, stwx;
    ls_row_stats<T, G>(x, K, tg, weight, conf, off, l, mx, se, stw, stwx);
    const T scale = g[0] / static_cast<T>(N);
    const T inv = stw / se;
    for (int k = l; k < K; k += G) {
        const T tw = (k == tg ? conf : off) * (weight ? weight[k] : static_cast<T>(1));
        gpred[(size_t)n * K + k] = scale * (t_exp<T>(x[k] - mx) * inv - tw);
    }
}

}  // namespace fc

namespace {

using fc::features_ok;

int launch_status() { return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH; }

int64_t blocks_for(int64_t items, int per_block) { return (items + per_block - 1) / per_block; }

template <typename T>
int twin_forward(const void* xS, int32_t nS, const void* xT, int32_t nT, int32_t C, const int64_t* p_, int64_t P, const int64_t* n_,
                 int64_t M, const void* yN, double mu, void* d2, void* loss, void* workspace, hipStream_t s) {
    const int64_t G = blocks_for(P + M, fc::kLossThreads);
    double* partials = static_cast<double*>(workspace);
    hipLaunchKernelGGL(fc::twin_forward_kernel<T>, dim3((unsigned)G), dim3(fc::kLossThreads), 0, s, static_cast<const T*>(xS), nS,
                       static_cast<const T*>(xT), nT, C, p_, P, n_, M, static_cast<const float*>(yN), static_cast<T>(mu), static_cast<T*>(d2),
                       partials, static_cast<T*>(loss));
    if (G > 1)
        hipLaunchKernelGGL(fc::final_sum_kernel<T>, dim3(1), dim3(fc::kLossThreads), 0, s, partials, (int)G, (double)P, (double)M,
                           static_cast<T*>(loss));
    return launch_status();
}

template <typename T>
int twin_backward(const void* xS, int32_t nS, const void* xT, int32_t nT, int32_t C, const int64_t* p_, int64_t P, const int64_t* n_,
                  int64_t M, const void* yN, double mu, const void* d2, const void* g, const int64_t* rowptrT, const int64_t* orderT,
                  const int64_t* rowptrS, const int64_t* orderS, void* gT, void* gS, hipStream_t s) {
    const int64_t rows = (int64_t)nT + nS;
#define FC_TWIN_BWD(G)                                                                                                                  \
    hipLaunchKernelGGL((fc::twin_backward_kernel<T, G>), dim3((unsigned)blocks_for(rows, fc::kGradThreads / G)), dim3(fc::kGradThreads), 0, \
                       s, static_cast<const T*>(xS), nS, static_cast<const T*>(xT), nT, C, p_, P, n_, M, static_cast<const float*>(yN), \
                       static_cast<T>(mu), static_cast<const T*>(d2), static_cast<const T*>(g), rowptrT, orderT, rowptrS, orderS,       \
                       static_cast<T*>(gT), static_cast<T*>(gS))
    if (C <= 16) FC_TWIN_BWD(16);
    else FC_TWIN_BWD(64);
#undef FC_TWIN_BWD
    return launch_status();
}

template <typename T>
int count_dense(const void* xS, int32_t nS, const void* xT, int32_t nT, int32_t C, const double* thresholds, int32_t n_thr, int64_t* counts,
                hipStream_t s) {
    fc::DenseThresholds<T> thr;
    for (int t = 0; t < fc::kDenseMaxThr; ++t) thr.v[t] = t < n_thr ? static_cast<T>(thresholds[t]) : static_cast<T>(INFINITY);
    const int64_t tilesS = blocks_for(nS, fc::kDenseTile), tiles = tilesS * blocks_for(nT, fc::kDenseTile);
    const unsigned grid = (unsigned)(tiles < fc::kDenseMaxGrid ? tiles : fc::kDenseMaxGrid);
    if (hipMemsetAsync(counts, 0, 2 * (size_t)n_thr * sizeof(int64_t), s) != hipSuccess) return FC_ERR_LAUNCH;
#define FC_DENSE(NT)                                                                                                              \
    hipLaunchKernelGGL((fc::twin_count_dense_kernel<T, NT>), dim3(grid), dim3(fc::kDenseThreads), 0, s, static_cast<const T*>(xS), nS, \
                       static_cast<const T*>(xT), nT, C, thr, n_thr, tilesS, tiles, reinterpret_cast<unsigned long long*>(counts))
    if (n_thr == 1) FC_DENSE(1);
    else if (n_thr <= 4) FC_DENSE(4);
    else FC_DENSE(16);
#undef FC_DENSE
    return launch_status();
}

bool smoothing_ok(const void* pred, const int64_t* target, int64_t N, int32_t K, int32_t dtype) {
    return pred && target && N >= 1 && K >= 1 && (dtype == 0 || dtype == 1) && (uint64_t)N * (uint64_t)K < ((uint64_t)1 << 40);
}

template <typename T>
int smoothing_forward(const void* pred, const int64_t* target, const void* weight, int64_t N, int32_t K, double conf, double off,
                      void* loss, void* workspace, hipStream_t s) {
    double* partials = static_cast<double*>(workspace);
    const int per_block = K <= 32 ? fc::kLossThreads : fc::kLossThreads / 64;
    const int64_t G = blocks_for(N, per_block);
#define FC_LS_FWD(GL)                                                                                                                      \
    hipLaunchKernelGGL((fc::label_smoothing_forward_kernel<T, GL>), dim3((unsigned)G), dim3(fc::kLossThreads), 0, s,                         \
                       static_cast<const T*>(pred), target, static_cast<const T*>(weight), N, K, static_cast<T>(conf), static_cast<T>(off), \
                       partials, static_cast<T*>(loss))
    if (K <= 32) FC_LS_FWD(1);
    else FC_LS_FWD(64);
#undef FC_LS_FWD
    if (G > 1)
        hipLaunchKernelGGL(fc::final_sum_kernel<T>, dim3(1), dim3(fc::kLossThreads), 0, s, partials, (int)G, (double)N, 1.0,
                           static_cast<T*>(loss));
    return launch_status();
}

template <typename T>
int smoothing_backward(const void* pred, const int64_t* target, const void* weight, const void* g, int64_t N, int32_t K, double conf,
                       double off, void* gpred, hipStream_t s) {
    const int per_block = K <= 32 ? fc::kLossThreads : fc::kLossThreads / 64;
#define FC_LS_BWD(GL)                                                                                                                     \
    hipLaunchKernelGGL((fc::label_smoothing_backward_kernel<T, GL>), dim3((unsigned)blocks_for(N, per_block)), dim3(fc::kLossThreads), 0, s, \
                       static_cast<const T*>(pred), target, static_cast<const T*>(weight), static_cast<const T*>(g), N, K,                \
                       static_cast<T>(conf), static_cast<T>(off), static_cast<T*>(gpred))
    if (K <= 32) FC_LS_BWD(1);
    else FC_LS_BWD(64);
#undef FC_LS_BWD
    return launch_status();
}

}  // namespace

extern "C" {

int fc_pair_sqdist(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* pairs, int64_t K,
                   void* d2, void* stream) {
    if (!features_ok(xS, N_S, xT, N_T, C, dtype) || K < 0 || K >= ((int64_t)1 << 39)) return FC_ERR_BAD_ARGUMENT;
    if (K == 0) return FC_OK;
    if (!pairs || !d2) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)blocks_for(K, 256));
    if (dtype == 0)
        hipLaunchKernelGGL(fc::pair_sqdist_kernel<float>, grid, dim3(256), 0, s, static_cast<const float*>(xS),
                           static_cast<const float*>(xT), pairs, K, C, static_cast<float*>(d2));
    else
        hipLaunchKernelGGL(fc::pair_sqdist_kernel<double>, grid, dim3(256), 0, s, static_cast<const double*>(xS),
                           static_cast<const double*>(xT), pairs, K, C, static_cast<double*>(d2));
    return launch_status();
}

size_t fc_twin_loss_workspace_bytes(int64_t P, int64_t M) {
    if (P < 1 || M < 1) return 0;
    return fc::align256((size_t)blocks_for(P + M, fc::kLossThreads) * 2 * sizeof(double));
}

int fc_twin_loss_forward(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* p_, int64_t P,
                         const int64_t* n_, int64_t M, const void* yN, double mu, void* d2, void* loss, void* workspace,
                         size_t workspace_bytes, void* stream) {
    if (!features_ok(xS, N_S, xT, N_T, C, dtype) || !p_ || !n_ || !yN || !d2 || !loss || P < 1 || M < 1 || P + M >= ((int64_t)1 << 39))
        return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_twin_loss_workspace_bytes(P, M)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? twin_forward<float>(xS, N_S, xT, N_T, C, p_, P, n_, M, yN, mu, d2, loss, workspace, s)
                      : twin_forward<double>(xS, N_S, xT, N_T, C, p_, P, n_, M, yN, mu, d2, loss, workspace, s);
}

int fc_twin_loss_backward(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const int64_t* p_, int64_t P,
                          const int64_t* n_, int64_t M, const void* yN, double mu, const void* d2, const void* grad_loss,
                          const int64_t* rowptr_T, const int64_t* order_T, const int64_t* rowptr_S, const int64_t* order_S, void* grad_xT,
                          void* grad_xS, void* stream) {
    if (!features_ok(xS, N_S, xT, N_T, C, dtype) || !p_ || !n_ || !yN || !d2 || !grad_loss || !rowptr_T || !order_T || !rowptr_S ||
        !order_S || !grad_xT || !grad_xS || P < 1 || M < 1 || P + M >= ((int64_t)1 << 39))
        return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? twin_backward<float>(xS, N_S, xT, N_T, C, p_, P, n_, M, yN, mu, d2, grad_loss, rowptr_T, order_T, rowptr_S, order_S,
                                             grad_xT, grad_xS, s)
                      : twin_backward<double>(xS, N_S, xT, N_T, C, p_, P, n_, M, yN, mu, d2, grad_loss, rowptr_T, order_T, rowptr_S,
                                              order_S, grad_xT, grad_xS, s);
}

int fc_twin_count_dense(const void* xS, int32_t N_S, const void* xT, int32_t N_T, int32_t C, int32_t dtype, const double* thresholds,
                        int32_t n_thresholds, int64_t* counts, void* stream) {
    if (!features_ok(xS, N_S, xT, N_T, C, dtype) || !thresholds || !counts || n_thresholds < 1 || n_thresholds > fc::kDenseMaxThr)
        return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? count_dense<float>(xS, N_S, xT, N_T, C, thresholds, n_thresholds, counts, s)
                      : count_dense<double>(xS, N_S, xT, N_T, C, thresholds, n_thresholds, counts, s);
}

size_t fc_label_smoothing_workspace_bytes(int64_t N, int32_t K) {
    if (N < 1 || K < 1) return 0;
    return fc::align256((size_t)blocks_for(N, K <= 32 ? fc::kLossThreads : fc::kLossThreads / 64) * 2 * sizeof(double));
}

int fc_label_smoothing_forward(const void* pred, const int64_t* target, const void* weight, int64_t N, int32_t K, int32_t dtype,
                               double confidence, double off_value, void* loss, void* workspace, size_t workspace_bytes, void* stream) {
    if (!smoothing_ok(pred, target, N, K, dtype) || !loss) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_label_smoothing_workspace_bytes(N, K)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? smoothing_forward<float>(pred, target, weight, N, K, confidence, off_value, loss, workspace, s)
                      : smoothing_forward<double>(pred, target, weight, N, K, confidence, off_value, loss, workspace, s);
}

int fc_label_smoothing_backward(const void* pred, const int64_t* target, const void* weight, const void* grad_loss, int64_t N, int32_t K,
                                int32_t dtype, double confidence, double off_value, void* grad_pred, void* stream) {
    if (!smoothing_ok(pred, target, N, K, dtype) || !grad_loss || !grad_pred) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == 0 ? smoothing_backward<float>(pred, target, weight, grad_loss, N, K, confidence, off_value, grad_pred, s)
                      : smoothing_backward<double>(pred, target, weight, grad_loss, N, K, confidence, off_value, grad_pred, s);
}

}  // extern "C"
