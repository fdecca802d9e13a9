// TangentDropout: dropout of (N,C) features by a REAL mask, and the raw words of the generator it draws from (fc_philox.hpp).
//
// A tangent feature is a complex number in its own sample's frame.  Dropping re and im independently (nn.Dropout on the real
// view) rotates the survivor and breaks gauge equivariance; multiplying the whole complex entry by a real mask commutes with any
// change of frames.  With T = floor(p * 2^24) (the caller's, computed in double) and scale = fl(1 / (1 - p)) (the caller's double,
// rounded once to the feature's scalar type):
//
//   entry e is DROPPED iff (word >> 8) < T, word = word e & 3 of block e >> 2 of the draw (seed, step, stream): an integer compare
//   kept      y = scale * x, one multiplication per scalar (re and im each), rounded on its own
//   dropped   y = +0 (+0 +0j) exactly -- a select, not a product: an Inf or NaN entry is silenced too
//
//   element   (stream 0) e = n C + c in 64-bit arithmetic: one decision per entry; one Philox block serves four consecutive entries
//   channel   (stream 1) e = b C + c, b the mesh of row n by ptr: one decision per mesh and channel, a whole feature channel of a
//             mesh is silenced ("spatial dropout" of a mesh); every row of the mesh recomputes its mesh's blocks
//
// The decision is a function of (seed, step, stream, e) alone, so the result cannot depend on the launch geometry; the gradient is
// the same call on gy (the mask is real and never stored).  One launch, no atomics, no workspace: every entry is read and written
// by one thread.  step is the caller's value or what a device int64 holds at the time the kernel runs.
#include "../../include/fieldconv_hip.h"
#include "fc_philox.hpp"
#include "fc_segment.hpp"

namespace fc {

constexpr int kDropThreads = 256;
constexpr unsigned kDropMaxBlocks = 1u << 16;          // grid-stride beyond (2^26 entries in element mode): the decisions do not depend on the geometry

template <typename T> struct alignas(16) DropVec { T v[16 / sizeof(T)]; };

template <typename T> __device__ __forceinline__ T drop_apply(T v, bool keep, T scale) { return keep ? v * scale : (T)0; }

// S scalars per entry (1 real, 2 complex).  A thread owns the four entries of one Philox block: 16 S sizeof(T) / 4 contiguous
// bytes, moved as 16-byte pieces when vec (x and y on 16-byte boundaries; a quad then starts on one, whatever q), else scalar by
// scalar; the last, partial quad always goes scalar by scalar.
template <typename T, int S>
__global__ __launch_bounds__(kDropThreads) void dropout_element_kernel(const T* __restrict__ x, T* __restrict__ y, uint64_t total,
                                                                       uint32_t threshold, T scale, uint64_t seed, int64_t step,
                                                                       const int64_t* __restrict__ step_ptr, int vec) {
    constexpr int QS = 4 * S, VW = 16 / (int)sizeof(T), NV = QS / VW;
    using Vec = DropVec<T>;
    const uint32_t st = philox_step(step, step_ptr);
    const uint64_t quads = (total + 3) >> 2, stride = (uint64_t)gridDim.x * kDropThreads;
    for (uint64_t q = (uint64_t)blockIdx.x * kDropThreads + threadIdx.x; q < quads; q += stride) {
        const PhiloxBlock r = philox_draw(seed, q, st, kStreamElementDropout);
        const uint64_t e0 = q << 2;
        if (vec && e0 + 4 <= total) {
            const Vec* src = reinterpret_cast<const Vec*>(x + e0 * S);
            Vec* dst = reinterpret_cast<Vec*>(y + e0 * S);
            Vec u[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) u[i] = src[i];
#pragma unroll
            for (int i = 0; i < NV; ++i) {
#pragma unroll
                for (int j = 0; j < VW; ++j) u[i].v[j] = drop_apply(u[i].v[j], philox_bits24(r.w[(i * VW + j) / S]) >= threshold, scale);
            }
#pragma unroll
            for (int i = 0; i < NV; ++i) dst[i] = u[i];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (e0 + k >= total) break;
                const bool keep = philox_bits24(r.w[k]) >= threshold;
#pragma unroll
                for (int j = 0; j < S; ++j) y[(e0 + k) * S + j] = drop_apply(x[(e0 + k) * S + j], keep, scale);
            }
        }
    }
}

// A thread owns (row n, the j-th Philox block that mesh b's entries b C .. b C + C - 1 touch); J = (C + 3) / 4 + 1 blocks cover
// any alignment of b C, a thread whose block lies past the mesh's entries leaves before it draws.  ptr NULL: one mesh.
template <typename T, int S>
__global__ __launch_bounds__(kDropThreads) void dropout_channel_kernel(const T* __restrict__ x, T* __restrict__ y,
                                                                       const int64_t* __restrict__ ptr, int B, int N, int C, int J,
                                                                       uint32_t threshold, T scale, uint64_t seed, int64_t step,
                                                                       const int64_t* __restrict__ step_ptr) {
    const uint32_t st = philox_step(step, step_ptr);
    const uint64_t total = (uint64_t)N * (uint64_t)J, stride = (uint64_t)gridDim.x * kDropThreads;
    for (uint64_t t = (uint64_t)blockIdx.x * kDropThreads + threadIdx.x; t < total; t += stride) {
        const int n = (int)(t / (uint64_t)J), j = (int)(t - (uint64_t)n * (uint64_t)J);
        const int b = ptr != nullptr ? seg_mesh_of_row(ptr, B, N, n) : 0;
        const uint64_t base = (uint64_t)b * (uint64_t)C, q = (base >> 2) + (uint64_t)j;
        const uint64_t lo = max(q << 2, base), hi = min((q << 2) + 4, base + (uint64_t)C);
        if (lo >= hi) continue;
        const PhiloxBlock r = philox_draw(seed, q, st, kStreamChannelDropout);
        for (uint64_t e = lo; e < hi; ++e) {
            const bool keep = philox_bits24(philox_word(r, (uint32_t)e & 3u)) >= threshold;
            const size_t idx = ((size_t)n * (size_t)C + (size_t)(e - base)) * S;
#pragma unroll
            for (int k = 0; k < S; ++k) y[idx + k] = drop_apply(x[idx + k], keep, scale);
        }
    }
}

__global__ __launch_bounds__(kDropThreads) void philox_words_kernel(uint64_t seed, uint32_t c2, uint32_t c3, uint64_t first_block,
                                                                    int64_t n_blocks, uint32_t* __restrict__ out) {
    const uint64_t stride = (uint64_t)gridDim.x * kDropThreads;
    for (uint64_t i = (uint64_t)blockIdx.x * kDropThreads + threadIdx.x; i < (uint64_t)n_blocks; i += stride) {
        const PhiloxBlock r = philox_draw(seed, first_block + i, c2, c3);          // (the sum wraps at 2^64, as the counter does)
#pragma unroll
        for (int k = 0; k < 4; ++k) out[4 * i + k] = r.w[k];
    }
}

}  // namespace fc

namespace {

unsigned drop_blocks(uint64_t threads) {
    const uint64_t blocks = (threads + fc::kDropThreads - 1) / fc::kDropThreads;
    return (unsigned)(blocks < fc::kDropMaxBlocks ? blocks : fc::kDropMaxBlocks);
}

template <typename T, int S>
int dropout_launch(const void* x, void* y, int32_t N, int32_t C, int32_t mode, const int64_t* ptr, int32_t B, uint32_t threshold,
                   double scale, uint64_t seed, int64_t step, const int64_t* step_ptr, hipStream_t s) {
    const T* xs = static_cast<const T*>(x);
    T* ys = static_cast<T*>(y);
    if (mode == 0) {
        const uint64_t total = (uint64_t)N * (uint64_t)C;
        const int vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
        hipLaunchKernelGGL((fc::dropout_element_kernel<T, S>), dim3(drop_blocks((total + 3) >> 2)), dim3(fc::kDropThreads), 0, s, xs, ys, total,
                           threshold, (T)scale, seed, step, step_ptr, vec);
    } else {
        const int J = (C + 3) / 4 + 1;
        hipLaunchKernelGGL((fc::dropout_channel_kernel<T, S>), dim3(drop_blocks((uint64_t)N * (uint64_t)J)), dim3(fc::kDropThreads), 0, s, xs, ys,
                           ptr, B, N, C, J, threshold, (T)scale, seed, step, step_ptr);
    }
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

int fc_philox_words(uint64_t seed, uint64_t hi, uint64_t first_block, int64_t n_blocks, uint32_t* out, void* stream) {
    if (n_blocks < 0 || (n_blocks > 0 && !out)) return FC_ERR_BAD_ARGUMENT;
    if (n_blocks == 0) return FC_OK;
    hipLaunchKernelGGL(fc::philox_words_kernel, dim3(drop_blocks((uint64_t)n_blocks)), dim3(fc::kDropThreads), 0, static_cast<hipStream_t>(stream),
                       seed, (uint32_t)hi, (uint32_t)(hi >> 32), first_block, n_blocks, out);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_dropout(const void* x, void* y, int32_t N, int32_t C, int32_t dtype, int32_t is_complex, int32_t mode, const int64_t* ptr, int32_t B,
               uint32_t threshold, double scale, uint64_t seed, int64_t step, const int64_t* step_ptr, void* stream) {
    if (!fc::seg_shape_ok(N, B, C) || (dtype != FC_F32 && dtype != FC_F64) || (is_complex != 0 && is_complex != 1) || (mode != 0 && mode != 1) ||
        threshold > (1u << 24) || !(scale > 0) || (mode == 1 && B > 1 && !ptr))
        return FC_ERR_BAD_ARGUMENT;
    if (N == 0) return FC_OK;
    if (!x || !y || x == y) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (dtype == FC_F32)
        return is_complex ? dropout_launch<float, 2>(x, y, N, C, mode, ptr, B, threshold, scale, seed, step, step_ptr, s)
                          : dropout_launch<float, 1>(x, y, N, C, mode, ptr, B, threshold, scale, seed, step, step_ptr, s);
    return is_complex ? dropout_launch<double, 2>(x, y, N, C, mode, ptr, B, threshold, scale, seed, step, step_ptr, s)
                      : dropout_launch<double, 1>(x, y, N, C, mode, ptr, B, threshold, scale, seed, step, step_ptr, s);
}

}  // extern "C"
