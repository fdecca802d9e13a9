// Per-mesh pooling over a mini-batch of meshes (a disjoint union whose mesh b owns the rows ptr[b] .. ptr[b+1] - 1 of an (N,C)
// row-major tensor):  out[b,c] = reduce_{n in mesh b} v(x[n,c])  with v = softAbs for complex input (the classification read-out
// mean(softAbs(x), dim=0), reference classification.ipynb Net.forward, without |x| ever written out) or v = x for real input (the
// per-mesh mean of a per-vertex loss is the C = 1 case), reduce = mean or sum, and the VJPs.
//
// Two launches forward, one backward, no atomics; the summation order depends on (ptr, C) only, never on timing:
//
//   slots    mesh b owns the chunk slots base(b) .. base(b+1) - 1,  base(b) = ptr[b] / 64 + b  (integer division).  base is
//            strictly increasing and base(b+1) - base(b) = ptr[b+1]/64 - ptr[b]/64 + 1 >= ceil(n_b / 64), so every mesh has room
//            for its chunks, the slot count N/64 + B is known without reading ptr on the host, and a workgroup finds the mesh
//            of its slot by bisection on base -- the (mesh, chunk) table in closed form.  A chunk never straddles two meshes.
//   partial  workgroup (slot g, channel tile t), 4 wavefronts x 64 lanes, lane = channel 64 t + lane: chunk j = g - base(b)
//            covers the rows ptr[b] + 64 j .. + 63 (cut at ptr[b+1]); wavefront w adds the rows w, w + 4, w + 8, ... of the
//            chunk to a zero in ascending order; partial[g,c] = (a_0 + a_1) + (a_2 + a_3).  Slots past a mesh's last chunk
//            are neither written nor read.
//   finish   workgroup (mesh b, channel tile t), same shape: wavefront w adds the chunks j = w, w + 4, ... of the mesh to a
//            zero in ascending order; s = (s_0 + s_1) + (s_2 + s_3); out[b,c] = s (sum) or s / n_b (mean; 0 for an empty mesh).
//   backward one thread per entry: gx[n,c] = (g[b,c] or g[b,c] / n_b) * dv, dv = 1 (real) or x / |x| outside the origin box and
//            0 inside (fc_soft_abs_backward's rule); the mesh of a row by bisection on ptr.
//
// float32 input accumulates in float32, float64 in float64.  ptr is read on the device only; its entries are clamped to [0, N]
// (and to the previous bound) where they are used, so a malformed ptr gives meaningless sums but touches nothing outside
// the buffers.
#include "../../include/fieldconv_hip.h"
#include "fc_segment.hpp"
#include "fc_workspace.hpp"

namespace fc {

__device__ __forceinline__ float seg_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double seg_sqrt(double v) { return sqrt(v); }

// reference utils/field.py:10-16: both components strictly inside (-1e-7, 1e-7), whatever the dtype
template <typename T> __device__ __forceinline__ bool seg_origin(SegCx<T> z) {
    const T e = (T)1e-7;
    return z.x < e && z.x > -e && z.y < e && z.y > -e;
}

template <typename T, bool ABS> __device__ __forceinline__ T seg_value(const void* __restrict__ x, size_t idx) {
    if constexpr (ABS) {
        const SegCx<T> z = static_cast<const SegCx<T>*>(x)[idx];
        return seg_origin(z) ? (T)0 : seg_sqrt(z.x * z.x + z.y * z.y);
    } else {
        return static_cast<const T*>(x)[idx];
    }
}

template <typename T, bool ABS>
__global__ __launch_bounds__(kSegThreads) void segment_partial_kernel(const void* __restrict__ x, const int64_t* __restrict__ ptr, int B,
                                                                      int N, int C, T* __restrict__ partial) {
    __shared__ T acc[kSegWaves][64];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const int b = seg_mesh_of_slot(ptr, B, N, g);
    int p0, p1, r0, r1;
    seg_range(ptr, b, N, p0, p1);
    if (!seg_chunk_rows(g, b, p0, p1, r0, r1)) return;       // a spare slot (the whole workgroup leaves)
    T s = (T)0;
    if (c < C)
        for (int r = r0 + wave; r < r1; r += kSegWaves) s += seg_value<T, ABS>(x, (size_t)r * C + c);
    s = seg_combine(acc, s, wave, lane);
    if (wave == 0 && c < C) partial[(size_t)g * C + c] = s;
}

template <typename T>
__global__ __launch_bounds__(kSegThreads) void segment_finish_kernel(const T* __restrict__ partial, const int64_t* __restrict__ ptr, int N,
                                                                     int C, int mean, T* __restrict__ out) {
    __shared__ T acc[kSegWaves][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    int p0, p1;
    seg_range(ptr, b, N, p0, p1);
    const int n = p1 - p0, chunks = (n + kSegRows - 1) / kSegRows, base = p0 / kSegRows + b;
    T s = (T)0;
    if (c < C)
        for (int j = wave; j < chunks; j += kSegWaves) s += partial[(size_t)(base + j) * C + c];
    s = seg_combine(acc, s, wave, lane);
    if (wave == 0 && c < C) out[(size_t)b * C + c] = mean ? (n > 0 ? s / (T)n : (T)0) : s;
}

template <typename T, bool ABS>
__global__ __launch_bounds__(kSegThreads) void segment_backward_kernel(const void* __restrict__ x, const T* __restrict__ g,
                                                                       const int64_t* __restrict__ ptr, int B, int N, int C, int mean,
                                                                       void* __restrict__ gx) {
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
        const bool inside = r >= p0 && r < p1;
        T s = (T)0;
        if (inside) {
            s = g[(size_t)b * C + c];
            if (mean) s = s / (T)(p1 - p0);
        }
        const size_t idx = (size_t)r * C + c;
        if constexpr (ABS) {
            const SegCx<T> z = static_cast<const SegCx<T>*>(x)[idx];
            SegCx<T> o;
            o.x = (T)0;
            o.y = (T)0;
            if (inside && !seg_origin(z)) {
                const T q = s / seg_sqrt(z.x * z.x + z.y * z.y);
                o.x = z.x * q;
                o.y = z.y * q;
            }
            static_cast<SegCx<T>*>(gx)[idx] = o;
        } else {
            static_cast<T*>(gx)[idx] = s;
        }
    }
}

}  // namespace fc

namespace {

using fc::seg_slots;

bool seg_dims_ok(int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce) {
    return fc::seg_shape_ok(N, B, C) && (dtype == FC_F32 || dtype == FC_F64) && (reduce == 0 || reduce == 1);
}

template <typename T, bool ABS>
int seg_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t reduce, void* out, void* workspace,
                hipStream_t s) {
    const dim3 block(fc::kSegThreads);
    const unsigned tiles = (unsigned)((C + 63) / 64);
    T* partial = static_cast<T*>(workspace);
    hipLaunchKernelGGL((fc::segment_partial_kernel<T, ABS>), dim3((unsigned)seg_slots(N, B), tiles), block, 0, s, x, ptr, B, N, C, partial);
    hipLaunchKernelGGL((fc::segment_finish_kernel<T>), dim3((unsigned)B, tiles), block, 0, s, partial, ptr, N, C, reduce == 0 ? 1 : 0,
                       static_cast<T*>(out));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T, bool ABS>
int seg_backward(const void* x, const void* g, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t reduce, void* gx,
                 hipStream_t s) {
    if (N == 0) return FC_OK;
    const unsigned tiles = (unsigned)((C + 63) / 64);
    hipLaunchKernelGGL((fc::segment_backward_kernel<T, ABS>), dim3((unsigned)((N + fc::kSegRows - 1) / fc::kSegRows), tiles),
                       dim3(fc::kSegThreads), 0, s, x, static_cast<const T*>(g), ptr, B, N, C, reduce == 0 ? 1 : 0, gx);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t fc_segment_pool_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t dtype) {
    if (!seg_dims_ok(N, B, C, dtype, 0)) return 0;
    return fc::align256((size_t)seg_slots(N, B) * (size_t)C * (dtype == FC_F64 ? 8 : 4));
}

int fc_segment_pool_soft_abs_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce,
                                     void* out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!seg_dims_ok(N, B, C, dtype, reduce) || !ptr || !out || (N > 0 && !x)) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_segment_pool_workspace_bytes(N, B, C, dtype)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? seg_forward<float, true>(x, ptr, N, B, C, reduce, out, workspace, s)
                           : seg_forward<double, true>(x, ptr, N, B, C, reduce, out, workspace, s);
}

int fc_segment_pool_soft_abs_backward(const void* x, const void* grad_out, const int64_t* ptr, int32_t N, int32_t B, int32_t C,
                                      int32_t dtype, int32_t reduce, void* grad_x, void* stream) {
    if (!seg_dims_ok(N, B, C, dtype, reduce) || !ptr || !grad_out || (N > 0 && (!x || !grad_x))) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? seg_backward<float, true>(x, grad_out, ptr, N, B, C, reduce, grad_x, s)
                           : seg_backward<double, true>(x, grad_out, ptr, N, B, C, reduce, grad_x, s);
}

int fc_segment_pool_forward(const void* x, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce, void* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!seg_dims_ok(N, B, C, dtype, reduce) || !ptr || !out || (N > 0 && !x)) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_segment_pool_workspace_bytes(N, B, C, dtype)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? seg_forward<float, false>(x, ptr, N, B, C, reduce, out, workspace, s)
                           : seg_forward<double, false>(x, ptr, N, B, C, reduce, out, workspace, s);
}

int fc_segment_pool_backward(const void* grad_out, const int64_t* ptr, int32_t N, int32_t B, int32_t C, int32_t dtype, int32_t reduce,
                             void* grad_x, void* stream) {
    if (!seg_dims_ok(N, B, C, dtype, reduce) || !ptr || !grad_out || (N > 0 && !grad_x)) return FC_ERR_BAD_ARGUMENT;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? seg_backward<float, false>(nullptr, grad_out, ptr, N, B, C, reduce, grad_x, s)
                           : seg_backward<double, false>(nullptr, grad_out, ptr, N, B, C, reduce, grad_x, s);
}

}  // extern "C"
