// TangentNorm: per-mesh normalisation of tangent features over a mini-batch of meshes (mesh b owns the rows ptr[b] .. ptr[b+1] - 1
// of an (N,C) row-major complex tensor).  Every channel of every mesh is scaled by the reciprocal root of its (weighted) mean
// squared magnitude; no mean is subtracted -- a tangent feature is a complex number in its own sample's frame, a mean over
// samples would mix frames -- so the layer touches magnitudes only and commutes with any change of frames:
//
//   W[b]   = sum_{n in b} w[n]                                              (w = 1 without weights: W[b] = n_b)
//   m[b,c] = sum_{n in b} w[n] |x[n,c]|^2 / W[b]                            (0 where W[b] == 0, and for an empty mesh)
//   r[b,c] = 1 / sqrt(m[b,c] + eps)
//   y[n,c] = gain[c] r[b,c] x[n,c]
//   t[b,c] = sum_{n in b} re(x) re(gy) + im(x) im(gy)
//   gx[n,c]  = gain[c] r[b,c] gy[n,c] - gain[c] r[b,c]^3 t[b,c] (w[n] / W[b]) x[n,c]      (second term 0 where W[b] == 0)
//   ggain[c] = sum_b r[b,c] t[b,c]                                          (b ascending)
//
// Both passes are "segmented reduction to (B,C), then a pass over (N,C)" on fc_segment.hip's chunk-slot scheme (fc_segment.hpp):
//
//   partial  workgroup (slot g, channel tile t), 4 wavefronts x 64 lanes, lane = channel 64 t + lane: wavefront v adds the terms
//            of the rows v, v + 4, ... of the chunk to a zero in ascending order, partial[g,c] = (a_0 + a_1) + (a_2 + a_3); the
//            terms are w |x|^2 (forward) or <x, gy> (backward).  With weights, the workgroups of tile 0 add w over the chunk in
//            the same order: wsum[g].
//   finish   workgroup (mesh b, channel tile t): wavefront v adds the chunks v, v + 4, ... of the mesh, s = (s_0 + s_1) + (s_2 + s_3),
//            W the same way from wsum (every tile computes the same W); forward writes r[b,c], backward t[b,c] and W[b].
//   apply    workgroup (64 rows, channel tile t): the mesh of a row by bisection on ptr; y or gx.
//   gain     backward only, when ggain is wanted: one thread per channel adds r t over b ascending.
//
// Three launches forward, three or four backward, no atomics; the order of every sum depends on the mesh's own row count and on
// C only, so a mesh inside a batch gets the bits it gets alone.  r is written out forward and read backward: the statistic is
// not recomputed (W, a sum over w alone, is).  float32 input accumulates in float32, float64 in float64.  ptr entries are
// clamped to [0, N] where they are read; a row that a malformed ptr leaves in no mesh is written as zero.
#include "../../include/fieldconv_hip.h"
#include "fc_segment.hpp"
#include "fc_workspace.hpp"

namespace fc {

__device__ __forceinline__ float norm_rsqrt(float v) { return 1.0f / sqrtf(v); }
__device__ __forceinline__ double norm_rsqrt(double v) { return 1.0 / sqrt(v); }

// BACKWARD false: the terms w |x|^2; true: <x, gy>.  wsum is written only where w is given.
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(kSegThreads) void norm_partial_kernel(const SegCx<T>* __restrict__ x, const SegCx<T>* __restrict__ gy,
                                                                   const T* __restrict__ w, const int64_t* __restrict__ ptr, int B, int N,
                                                                   int C, T* __restrict__ partial, T* __restrict__ wsum) {
    __shared__ T acc[kSegWaves][64];
    __shared__ T wacc[kSegWaves][64];
    const int g = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    const int b = seg_mesh_of_slot(ptr, B, N, g);
    int p0, p1, r0, r1;
    seg_range(ptr, b, N, p0, p1);
    if (!seg_chunk_rows(g, b, p0, p1, r0, r1)) return;       // a spare slot (the whole workgroup leaves)
    const bool weigh = w != nullptr && blockIdx.y == 0;      // uniform over the workgroup
    T s = (T)0, sw = (T)0;
    for (int r = r0 + wave; r < r1; r += kSegWaves) {
        T wn = (T)1;
        if (w != nullptr) wn = w[r];
        if (weigh) sw += wn;
        if (c < C) {
            const size_t idx = (size_t)r * C + c;
            const SegCx<T> z = x[idx];
            if constexpr (BACKWARD) {
                const SegCx<T> q = gy[idx];
                s += z.x * q.x + z.y * q.y;
            } else {
                s += wn * (z.x * z.x + z.y * z.y);
            }
        }
    }
    s = seg_combine(acc, s, wave, lane);
    if (wave == 0 && c < C) partial[(size_t)g * C + c] = s;
    if (weigh) {
        sw = seg_combine(wacc, sw, wave, lane);
        if (threadIdx.x == 0) wsum[g] = sw;
    }
}

// forward (BACKWARD false): out = r (B,C); backward: out = t (B,C) and wtot = W (B)
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(kSegThreads) void norm_finish_kernel(const T* __restrict__ partial, const T* __restrict__ wsum,
                                                                  const int64_t* __restrict__ ptr, int N, int C, T eps, T* __restrict__ out,
                                                                  T* __restrict__ wtot) {
    __shared__ T acc[kSegWaves][64];
    __shared__ T wacc[kSegWaves][64];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    int p0, p1;
    seg_range(ptr, b, N, p0, p1);
    const int n = p1 - p0, chunks = (n + kSegRows - 1) / kSegRows, base = p0 / kSegRows + b;
    T s = (T)0, sw = (T)0;
    for (int j = wave; j < chunks; j += kSegWaves) {
        if (c < C) s += partial[(size_t)(base + j) * C + c];
        if (wsum != nullptr) sw += wsum[base + j];
    }
    s = seg_combine(acc, s, wave, lane);
    const T W = wsum != nullptr ? seg_combine(wacc, sw, wave, lane) : (T)n;
    if (wave != 0) return;
    if constexpr (BACKWARD) {
        if (c < C) out[(size_t)b * C + c] = s;
        if (threadIdx.x == 0 && blockIdx.y == 0) wtot[b] = W;
    } else {
        if (c < C) out[(size_t)b * C + c] = norm_rsqrt((W > (T)0 ? s / W : (T)0) + eps);
    }
}

// forward: y = (gain r) x.  backward (v = gy): gx = (gain r) gy - ((gain r) (r r) t (w / W)) x
template <typename T, bool BACKWARD>
__global__ __launch_bounds__(kSegThreads) void norm_apply_kernel(const SegCx<T>* __restrict__ x, const SegCx<T>* __restrict__ gy,
                                                                 const T* __restrict__ w, const int64_t* __restrict__ ptr,
                                                                 const T* __restrict__ gain, const T* __restrict__ rr, const T* __restrict__ tt,
                                                                 const T* __restrict__ wtot, int B, int N, int C, SegCx<T>* __restrict__ out) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.y * 64 + lane;
    if (c >= C) return;
    const T gn = gain != nullptr ? gain[c] : (T)1;
    const int rend = (int)min((long long)N, ((long long)blockIdx.x + 1) * kSegRows);
    int b = 0, p0 = 0, p1 = 0;
    bool have = false;
    T a = (T)0, k = (T)0, W = (T)0;
    for (int r = blockIdx.x * kSegRows + wave; r < rend; r += kSegWaves) {
        if (!have || r >= p1) {                              // rows ascend: look the mesh up again only past the current one's end
            b = seg_mesh_of_row(ptr, B, N, r);
            seg_range(ptr, b, N, p0, p1);
            have = true;
            const T rb = rr[(size_t)b * C + c];
            a = gn * rb;
            if constexpr (BACKWARD) {
                W = wtot[b];
                k = a * (rb * rb) * tt[(size_t)b * C + c];
            }
        }
        const size_t idx = (size_t)r * C + c;
        SegCx<T> o;
        o.x = (T)0;
        o.y = (T)0;
        if (r >= p0 && r < p1) {
            const SegCx<T> z = x[idx];
            if constexpr (BACKWARD) {
                const SegCx<T> q = gy[idx];
                o.x = a * q.x;
                o.y = a * q.y;
                if (W > (T)0) {
                    const T f = k * ((w != nullptr ? w[r] : (T)1) / W);
                    o.x -= f * z.x;
                    o.y -= f * z.y;
                }
            } else {
                o.x = a * z.x;
                o.y = a * z.y;
            }
        }
        out[idx] = o;
    }
}

template <typename T>
__global__ void norm_gain_kernel(const T* __restrict__ rr, const T* __restrict__ tt, int B, int C, T* __restrict__ ggain) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    T s = (T)0;
    for (int b = 0; b < B; ++b) s += rr[(size_t)b * C + c] * tt[(size_t)b * C + c];
    ggain[c] = s;
}

}  // namespace fc

namespace {

using fc::seg_slots;

bool norm_dims_ok(int32_t N, int32_t B, int32_t C, int32_t dtype) { return fc::seg_shape_ok(N, B, C) && (dtype == FC_F32 || dtype == FC_F64); }

// workspace: partial (slots, C) | wsum (slots) | t (B, C) | W (B), each rounded up to 256 bytes; the forward pass uses the first two
template <typename T>
struct NormWorkspace { T *partial, *wsum, *t, *wtot; };
template <typename T>
NormWorkspace<T> norm_workspace(fc::Carver& c, int32_t N, int32_t B, int32_t C) {
    const size_t slots = (size_t)seg_slots(N, B);
    return {c.take<T>(slots * (size_t)C * sizeof(T)), c.take<T>(slots * sizeof(T)), c.take<T>((size_t)B * (size_t)C * sizeof(T)),
            c.take<T>((size_t)B * sizeof(T))};
}

template <typename T>
int norm_forward(const void* x, const void* w, const int64_t* ptr, const void* gain, int32_t N, int32_t B, int32_t C, double eps, void* y,
                 void* r, void* workspace, hipStream_t s) {
    fc::Carver c(workspace);
    const NormWorkspace<T> ws = norm_workspace<T>(c, N, B, C);
    T *partial = ws.partial, *wsum = w ? ws.wsum : nullptr;             // (wsum takes room whether or not there are weights)
    const auto* xc = static_cast<const fc::SegCx<T>*>(x);
    const T* wt = static_cast<const T*>(w);
    const dim3 block(fc::kSegThreads);
    const unsigned tiles = (unsigned)((C + 63) / 64);
    hipLaunchKernelGGL((fc::norm_partial_kernel<T, false>), dim3((unsigned)seg_slots(N, B), tiles), block, 0, s, xc, nullptr, wt, ptr, B, N, C,
                       partial, wsum);
    hipLaunchKernelGGL((fc::norm_finish_kernel<T, false>), dim3((unsigned)B, tiles), block, 0, s, partial, wsum, ptr, N, C, (T)eps,
                       static_cast<T*>(r), nullptr);
    if (N > 0)
        hipLaunchKernelGGL((fc::norm_apply_kernel<T, false>), dim3((unsigned)((N + fc::kSegRows - 1) / fc::kSegRows), tiles), block, 0, s, xc,
                           nullptr, wt, ptr, static_cast<const T*>(gain), static_cast<const T*>(r), nullptr, nullptr, B, N, C,
                           static_cast<fc::SegCx<T>*>(y));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

template <typename T>
int norm_backward(const void* x, const void* w, const int64_t* ptr, const void* gain, const void* r, const void* gy, int32_t N, int32_t B,
                  int32_t C, void* gx, void* ggain, void* workspace, hipStream_t s) {
    fc::Carver c(workspace);
    const NormWorkspace<T> ws = norm_workspace<T>(c, N, B, C);
    T *partial = ws.partial, *wsum = w ? ws.wsum : nullptr, *t = ws.t, *wtot = ws.wtot;
    const auto* xc = static_cast<const fc::SegCx<T>*>(x);
    const auto* gc = static_cast<const fc::SegCx<T>*>(gy);
    const T* wt = static_cast<const T*>(w);
    const dim3 block(fc::kSegThreads);
    const unsigned tiles = (unsigned)((C + 63) / 64);
    hipLaunchKernelGGL((fc::norm_partial_kernel<T, true>), dim3((unsigned)seg_slots(N, B), tiles), block, 0, s, xc, gc, wt, ptr, B, N, C, partial,
                       wsum);
    hipLaunchKernelGGL((fc::norm_finish_kernel<T, true>), dim3((unsigned)B, tiles), block, 0, s, partial, wsum, ptr, N, C, (T)0, t, wtot);
    if (N > 0 && gx)
        hipLaunchKernelGGL((fc::norm_apply_kernel<T, true>), dim3((unsigned)((N + fc::kSegRows - 1) / fc::kSegRows), tiles), block, 0, s, xc, gc,
                           wt, ptr, static_cast<const T*>(gain), static_cast<const T*>(r), t, wtot, B, N, C, static_cast<fc::SegCx<T>*>(gx));
    if (ggain)
        hipLaunchKernelGGL((fc::norm_gain_kernel<T>), dim3((unsigned)((C + 255) / 256)), dim3(256), 0, s, static_cast<const T*>(r), t, B, C,
                           static_cast<T*>(ggain));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // namespace

extern "C" {

size_t fc_tangent_norm_workspace_bytes(int32_t N, int32_t B, int32_t C, int32_t dtype) {
    if (!norm_dims_ok(N, B, C, dtype)) return 0;
    return dtype == FC_F64 ? fc::carved_bytes(norm_workspace<double>, N, B, C) : fc::carved_bytes(norm_workspace<float>, N, B, C);
}

int fc_tangent_norm_forward(const void* x, const void* w, const int64_t* ptr, const void* gain, int32_t N, int32_t B, int32_t C, int32_t dtype,
                            double eps, void* y, void* r, void* workspace, size_t workspace_bytes, void* stream) {
    if (!norm_dims_ok(N, B, C, dtype) || !ptr || !r || !(eps >= 0) || (N > 0 && (!x || !y))) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_tangent_norm_workspace_bytes(N, B, C, dtype)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? norm_forward<float>(x, w, ptr, gain, N, B, C, eps, y, r, workspace, s)
                           : norm_forward<double>(x, w, ptr, gain, N, B, C, eps, y, r, workspace, s);
}

int fc_tangent_norm_backward(const void* x, const void* w, const int64_t* ptr, const void* gain, const void* r, const void* gy, int32_t N,
                             int32_t B, int32_t C, int32_t dtype, void* gx, void* ggain, void* workspace, size_t workspace_bytes,
                             void* stream) {
    if (!norm_dims_ok(N, B, C, dtype) || !ptr || !r || (N > 0 && (!x || !gy)) || (!gx && !ggain)) return FC_ERR_BAD_ARGUMENT;
    if (!workspace || workspace_bytes < fc_tangent_norm_workspace_bytes(N, B, C, dtype)) return FC_ERR_WORKSPACE;
    hipStream_t s = static_cast<hipStream_t>(stream);
    return dtype == FC_F32 ? norm_backward<float>(x, w, ptr, gain, r, gy, N, B, C, gx, ggain, workspace, s)
                           : norm_backward<double>(x, w, ptr, gain, r, gy, N, B, C, gx, ggain, workspace, s);
}

}  // extern "C"
