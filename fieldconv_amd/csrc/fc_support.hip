// Support-graph construction on the device (the preprocessing the reference does with torch_cluster through PyG):
//   fc_fps                       farthest-point sampling, one 1024-thread workgroup, one dependent argmax round per sample;
//   fc_radius_count / _fill      every point's neighbours within epsilon, at most K of them (the K nearest, ties to the
//                                lower index), as (E,2) int64 [query, neighbour] rows grouped by query, neighbours ascending.
//   fc_fps_batched, fc_radius_count_batched / _fill_batched      the same over a mini-batch of point sets (mesh b owns the rows
//                                ptr[b] .. ptr[b+1] - 1 of pos): one FPS workgroup per mesh, and a radius search that looks for a
//                                query's neighbours inside the query's own mesh only.
// Both use one squared-distance formula, d2 = (dx*dx + dy*dy) + dz*dz with dx = p_n.x - p_q.x, each operation rounded on its
// own (no contraction), so that numpy float32 evaluates exactly the same numbers.
#include <hipcub/hipcub.hpp>
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_workspace.hpp"

namespace fc {

constexpr int kFpsThreads = 1024;           // one workgroup: point i belongs to thread i % 1024
constexpr int kFpsWaves = kFpsThreads / 64;
constexpr int kFpsRegPoints = 16;           // points per thread held in registers (N <= 16384); the rest in the workspace
constexpr int kRadiusThreads = 256;         // queries per workgroup of the count / fill kernels = candidates per LDS tile

__device__ __forceinline__ float sq_dist(float qx, float qy, float qz, float nx, float ny, float nz) {
#pragma clang fp contract(off)          // (plain operators: __fmul_rn / __fadd_rn are header functions that hipcc contracts)
    const float dx = nx - qx, dy = ny - qy, dz = nz - qz;
    return (dx * dx + dy * dy) + dz * dz;
}

// Selection key of an unselected point: larger distance first, then lower index.  A selected point carries 0, below every
// unselected point's key (~i has its top bit set for i < 2^31).
__device__ __forceinline__ uint64_t fps_key(float mind, int i) {
    return mind < 0.f ? 0ull : ((uint64_t)__float_as_uint(mind) << 32) | (uint64_t)(~(uint32_t)i);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint64_t o = __shfl_xor((unsigned long long)v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

// One workgroup samples one point set.  mind < 0 marks a selected point: fminf keeps it negative for good.
__device__ __forceinline__ void fps_body(const float* __restrict__ pos, int N, int S, int start, int64_t* __restrict__ idx,
                                         float* __restrict__ mind_ws, uint64_t (*slots)[kFpsWaves]) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    float rx[kFpsRegPoints], ry[kFpsRegPoints], rz[kFpsRegPoints], rm[kFpsRegPoints];
#pragma unroll
    for (int j = 0; j < kFpsRegPoints; ++j) {
        const int i = t + j * kFpsThreads;
        const bool in = i < N;
        rx[j] = in ? pos[3 * (size_t)i] : 0.f;
        ry[j] = in ? pos[3 * (size_t)i + 1] : 0.f;
        rz[j] = in ? pos[3 * (size_t)i + 2] : 0.f;
        rm[j] = in ? __int_as_float(0x7f800000) : -1.f;          // +inf; padding counts as selected
    }
    for (int i = t + kFpsRegPoints * kFpsThreads; i < N; i += kFpsThreads) mind_ws[i] = __int_as_float(0x7f800000);
    if (t == 0) idx[0] = start;
    int last = start;
    for (int k = 1; k < S; ++k) {
        const float qx = pos[3 * (size_t)last], qy = pos[3 * (size_t)last + 1], qz = pos[3 * (size_t)last + 2];
        uint64_t best = 0;
#pragma unroll
        for (int j = 0; j < kFpsRegPoints; ++j) {
            const int i = t + j * kFpsThreads;
            const float d = sq_dist(qx, qy, qz, rx[j], ry[j], rz[j]);
            rm[j] = i == last ? -1.f : fminf(rm[j], d);
            const uint64_t key = fps_key(rm[j], i);
            best = key > best ? key : best;
        }
        for (int i = t + kFpsRegPoints * kFpsThreads; i < N; i += kFpsThreads) {
            const float d = sq_dist(qx, qy, qz, pos[3 * (size_t)i], pos[3 * (size_t)i + 1], pos[3 * (size_t)i + 2]);
            const float m = i == last ? -1.f : fminf(mind_ws[i], d);
            mind_ws[i] = m;
            const uint64_t key = fps_key(m, i);
            best = key > best ? key : best;
        }
        best = wave_max_u64(best);
        // slots alternate with the round's parity: a wave can only write this round's buffer again two rounds on, after
        // the next barrier, which every wave reaches only once it has read this round's slots
        if (lane == 0) slots[k & 1][wave] = best;
        __syncthreads();
        uint64_t win = slots[k & 1][0];
#pragma unroll
        for (int w = 1; w < kFpsWaves; ++w) {
            const uint64_t o = slots[k & 1][w];
            win = o > win ? o : win;
        }
        last = (int)(~(uint32_t)win);
        if (t == 0) idx[k] = last;
    }
}

__global__ __launch_bounds__(kFpsThreads) void fps_kernel(const float* __restrict__ pos, int N, int S, int start,
                                                          int64_t* __restrict__ idx, float* __restrict__ mind_ws) {
    __shared__ uint64_t slots[2][kFpsWaves];
    fps_body(pos, N, S, start, idx, mind_ws, slots);
}

// ptr entry b clamped to [0, N]: a malformed table can give a meaningless result, never an access outside pos
__device__ __forceinline__ int mesh_bound(const int64_t* __restrict__ ptr, int b, int N) {
    const int64_t v = ptr[b];
    return (int)(v < 0 ? 0 : (v > N ? N : v));
}

// Workgroup b samples mesh b: rows pos_ptr[b] .. pos_ptr[b+1] - 1 of pos, n_samples[b] of them from start[b], written to
// idx[out_ptr[b] ..] as indices LOCAL to the mesh.  The workspace slice of a mesh starts at its first point.  Whatever the
// tables hold, a mesh writes inside [0, S_total) and reads inside its own rows (a mesh whose samples do not fit is skipped).
__global__ __launch_bounds__(kFpsThreads) void fps_batched_kernel(const float* __restrict__ pos, const int64_t* __restrict__ pos_ptr, int N,
                                                                  const int64_t* __restrict__ n_samples, const int64_t* __restrict__ start,
                                                                  const int64_t* __restrict__ out_ptr, int64_t S_total,
                                                                  int64_t* __restrict__ idx, float* __restrict__ mind_ws) {
    __shared__ uint64_t slots[2][kFpsWaves];
    const int b = blockIdx.x;
    const int p0 = mesh_bound(pos_ptr, b, N), n = max(mesh_bound(pos_ptr, b + 1, N), p0) - p0;
    const int64_t S = n_samples[b], st = start[b], o = out_ptr[b];
    if (n < 1 || S < 1 || S > n || st < 0 || st >= n || o < 0 || o > S_total - S) return;
    fps_body(pos + 3 * (size_t)p0, n, (int)S, (int)st, idx + o, mind_ws + p0, slots);
}

// Stages candidates [tile, tile + kRadiusThreads) as float4 in LDS; the caller synchronises around it.
__device__ __forceinline__ void stage_tile(float4* tile_pos, const float* __restrict__ pos, int tile, int N) {
    const int n = tile + threadIdx.x;
    tile_pos[threadIdx.x] = n < N ? make_float4(pos[3 * (size_t)n], pos[3 * (size_t)n + 1], pos[3 * (size_t)n + 2], 0.f)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
}

// #{n in [0,N) : d2(q,n) < r2} for the workgroup's queries (one per thread; every thread of the workgroup calls this)
__device__ __forceinline__ int radius_count_body(float4* tile_pos, const float* __restrict__ pos, int N, int q, float r2) {
    const int qc = min(q, N - 1);
    const float qx = pos[3 * (size_t)qc], qy = pos[3 * (size_t)qc + 1], qz = pos[3 * (size_t)qc + 2];
    int c = 0;
    for (int tile = 0; tile < N; tile += kRadiusThreads) {
        __syncthreads();
        stage_tile(tile_pos, pos, tile, N);
        __syncthreads();
        const int m = min(kRadiusThreads, N - tile);
        for (int j = 0; j < m; ++j) {
            const float4 p = tile_pos[j];
            c += sq_dist(qx, qy, qz, p.x, p.y, p.z) < r2 ? 1 : 0;
        }
    }
    return c;
}

// count[q] = min(#{n : d2(q,n) < r2}, K) as int64 (the scan input; count[N] = 0 so that the scan's last entry is the total),
// overfull[q] = 1 when more than K points qualify.
__global__ __launch_bounds__(kRadiusThreads) void radius_count_kernel(const float* __restrict__ pos, int N, float r2, int K,
                                                                      int64_t* __restrict__ count, int32_t* __restrict__ overfull) {
    __shared__ float4 tile_pos[kRadiusThreads];
    const int q = blockIdx.x * kRadiusThreads + threadIdx.x;
    const int c = radius_count_body(tile_pos, pos, N, q, r2);
    if (q < N) {
        count[q] = min(c, K);
        overfull[q] = c > K ? 1 : 0;
    } else if (q == N) {
        count[N] = 0;
    }
}

// One wavefront per overfull query q of the point set pos (N points): the smallest t (a non-negative fp32 bit pattern) with
// #{d2 <= t} >= K, found by bisection on the 31 magnitude bits, and the quota K - #{d2 < t} of candidates at exactly t that
// are kept (the lowest indices).
__device__ __forceinline__ void radius_select_body(const float* __restrict__ pos, int N, int q, int lane, float r2, int K,
                                                   uint32_t* __restrict__ thresh, int32_t* __restrict__ quota) {
    const float qx = pos[3 * (size_t)q], qy = pos[3 * (size_t)q + 1], qz = pos[3 * (size_t)q + 2];
    auto count_le = [&](uint32_t t) {          // #{n : bits(d2) <= t}, wave total
        int c = 0;
        for (int n = lane; n < N; n += 64)
            c += __float_as_uint(sq_dist(qx, qy, qz, pos[3 * (size_t)n], pos[3 * (size_t)n + 1], pos[3 * (size_t)n + 2])) <= t ? 1 : 0;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) c += __shfl_xor(c, m, 64);
        return c;
    };
    // more than K points have d2 < r2, i.e. bits(d2) <= bits(r2) - 1: the answer lies in [0, bits(r2) - 1]
    uint32_t lo = 0, hi = __float_as_uint(r2) - 1u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (count_le(mid) >= K) hi = mid;
        else lo = mid + 1;
    }
    const int below = lo == 0 ? 0 : count_le(lo - 1);
    if (lane == 0) {
        *thresh = lo;
        *quota = K - below;
    }
}

// Queries that are not overfull return at once.
__global__ __launch_bounds__(256) void radius_select_kernel(const float* __restrict__ pos, int N, float r2, int K,
                                                            const int32_t* __restrict__ overfull, uint32_t* __restrict__ thresh,
                                                            int32_t* __restrict__ quota) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= N || !overfull[q]) return;
    radius_select_body(pos, N, q, lane, r2, K, thresh + q, quota + q);
}

// Same scan as the count kernel over the point set pos (N points); each lane walks the candidates of its query q in index
// order and writes its rows at its scanned offset.  Rows, and the per-query arrays, are numbered q + qbase / n + qbase.
__device__ __forceinline__ void radius_fill_body(float4* tile_pos, const float* __restrict__ pos, int N, int q, int qbase, float r2,
                                                 int64_t E, const int64_t* __restrict__ offsets, const int32_t* __restrict__ overfull,
                                                 const uint32_t* __restrict__ thresh, const int32_t* __restrict__ quota,
                                                 int64_t* __restrict__ edges) {
    const int qc = min(q, N - 1);
    const float qx = pos[3 * (size_t)qc], qy = pos[3 * (size_t)qc + 1], qz = pos[3 * (size_t)qc + 2];
    const int qg = q + qbase;
    const bool full = q < N && overfull[qg];
    const uint32_t t = full ? thresh[qg] : 0xffffffffu;
    int left_at_t = full ? quota[qg] : 0;
    // a non-overfull query keeps every d2 < r2: bits(d2) < 0xffffffff holds for all of them
    int64_t out = q < N ? offsets[qg] : 0;
    const int64_t end = q < N ? min(offsets[qg + 1], E) : 0;
    for (int tile = 0; tile < N; tile += kRadiusThreads) {
        __syncthreads();
        stage_tile(tile_pos, pos, tile, N);
        __syncthreads();
        const int m = min(kRadiusThreads, N - tile);
        for (int j = 0; j < m; ++j) {
            const float4 p = tile_pos[j];
            const float d = sq_dist(qx, qy, qz, p.x, p.y, p.z);
            if (!(d < r2)) continue;
            const uint32_t b = __float_as_uint(d);
            bool keep = b < t;
            if (b == t && left_at_t > 0) {
                keep = true;
                --left_at_t;
            }
            if (keep && out >= 0 && out < end) {
                edges[2 * out] = qg;
                edges[2 * out + 1] = tile + j + qbase;
                ++out;
            }
        }
    }
}

__global__ __launch_bounds__(kRadiusThreads) void radius_fill_kernel(const float* __restrict__ pos, int N, float r2, int64_t E,
                                                                     const int64_t* __restrict__ offsets, const int32_t* __restrict__ overfull,
                                                                     const uint32_t* __restrict__ thresh, const int32_t* __restrict__ quota,
                                                                     int64_t* __restrict__ edges) {
    __shared__ float4 tile_pos[kRadiusThreads];
    radius_fill_body(tile_pos, pos, N, blockIdx.x * kRadiusThreads + threadIdx.x, 0, r2, E, offsets, overfull, thresh, quota, edges);
}

// ---- the batched search: workgroups map to (mesh, query tile) pairs, so that the LDS candidate tile is always one mesh's.
// Mesh b owns the workgroup slots base(b) .. base(b+1) - 1 with base(b) = ptr[b] / 256 + b (integer division): base is strictly
// increasing and base(b+1) - base(b) = ptr[b+1]/256 - ptr[b]/256 + 1 >= ceil(n_b / 256), so N/256 + B workgroups suffice
// whatever ptr holds, and a workgroup finds its mesh by bisection on base -- the prefix table in closed form, nothing to build
// or to read back.  Slots past a mesh's last tile leave at once.  -> mesh rows [p0, p0 + n) and the tile's first local query.
__device__ __forceinline__ bool mesh_tile(const int64_t* __restrict__ ptr, int B, int N, int g, int& p0, int& n, int& q0) {
    int lo = 0, hi = B - 1;                                  // the largest b with base(b) <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mesh_bound(ptr, mid, N) / kRadiusThreads + mid <= g) lo = mid;
        else hi = mid - 1;
    }
    p0 = mesh_bound(ptr, lo, N);
    n = max(mesh_bound(ptr, lo + 1, N), p0) - p0;
    const long long first = (long long)(g - (p0 / kRadiusThreads + lo)) * kRadiusThreads;
    q0 = (int)min(max(first, 0ll), (long long)n);
    return first >= 0 && first < n;
}

__global__ __launch_bounds__(kRadiusThreads) void radius_count_batched_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                                              int B, int N, float r2, int K, int64_t* __restrict__ count,
                                                                              int32_t* __restrict__ overfull) {
    __shared__ float4 tile_pos[kRadiusThreads];
    if (blockIdx.x == 0 && threadIdx.x == 0) count[N] = 0;
    int p0, n, q0;
    if (!mesh_tile(ptr, B, N, blockIdx.x, p0, n, q0)) return;
    const int q = q0 + threadIdx.x;
    const int c = radius_count_body(tile_pos, pos + 3 * (size_t)p0, n, q, r2);
    if (q < n) {
        count[p0 + q] = min(c, K);
        overfull[p0 + q] = c > K ? 1 : 0;
    }
}

__global__ __launch_bounds__(256) void radius_select_batched_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr, int B,
                                                                    int N, float r2, int K, const int32_t* __restrict__ overfull,
                                                                    uint32_t* __restrict__ thresh, int32_t* __restrict__ quota) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= N || !overfull[q]) return;
    int lo = 0, hi = B - 1;                                  // the mesh of q: the largest b with ptr[b] <= q
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (mesh_bound(ptr, mid, N) <= q) lo = mid;
        else hi = mid - 1;
    }
    const int p0 = mesh_bound(ptr, lo, N), n = max(mesh_bound(ptr, lo + 1, N), p0) - p0;
    if (q < p0 || q >= p0 + n) return;
    radius_select_body(pos + 3 * (size_t)p0, n, q - p0, lane, r2, K, thresh + q, quota + q);
}

__global__ __launch_bounds__(kRadiusThreads) void radius_fill_batched_kernel(const float* __restrict__ pos, const int64_t* __restrict__ ptr,
                                                                             int B, int N, float r2, int64_t E,
                                                                             const int64_t* __restrict__ offsets,
                                                                             const int32_t* __restrict__ overfull,
                                                                             const uint32_t* __restrict__ thresh,
                                                                             const int32_t* __restrict__ quota, int64_t* __restrict__ edges) {
    __shared__ float4 tile_pos[kRadiusThreads];
    int p0, n, q0;
    if (!mesh_tile(ptr, B, N, blockIdx.x, p0, n, q0)) return;
    radius_fill_body(tile_pos, pos + 3 * (size_t)p0, n, q0 + threadIdx.x, p0, r2, E, offsets, overfull, thresh, quota, edges);
}

}  // namespace fc

namespace {

// radius workspace: count (N+1) int64 | offsets (N+1) int64 | overfull (N) int32 | thresh (N) uint32 | quota (N) int32 | scan scratch
struct RadiusWs { int64_t *count, *offsets; int32_t* overfull; uint32_t* thresh; int32_t* quota; void* scan; size_t scan_bytes; };
RadiusWs radius_ws(fc::Carver& c, int32_t N) {
    const size_t n = (size_t)N;
    RadiusWs w;
    w.count = c.take<int64_t>((n + 1) * 8);
    w.offsets = c.take<int64_t>((n + 1) * 8);
    w.overfull = c.take<int32_t>(n * 4);
    w.thresh = c.take<uint32_t>(n * 4);
    w.quota = c.take<int32_t>(n * 4);
    w.scan_bytes = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, w.scan_bytes, (const int64_t*)nullptr, (int64_t*)nullptr, N + 1);
    w.scan = c.take(w.scan_bytes);
    return w;
}
size_t radius_bytes(int32_t N) { return fc::carved_bytes(radius_ws, N); }

bool finite_positive(float x) { return x > 0.f && x <= 3.402823466e38f; }

}  // namespace

extern "C" {

size_t fc_fps_workspace_bytes(int32_t N) {
    if (N < 1) return 0;
    return fc::align256((size_t)N * 4);
}

int fc_fps(const float* pos, int32_t N, int32_t n_samples, int32_t start, int64_t* idx, void* workspace, size_t workspace_bytes,
           void* stream) {
    if (!pos || !idx || !workspace || N < 1 || n_samples < 1 || n_samples > N || start < 0 || start >= N) return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < fc_fps_workspace_bytes(N)) return FC_ERR_WORKSPACE;
    hipLaunchKernelGGL(fc::fps_kernel, dim3(1), dim3(fc::kFpsThreads), 0, static_cast<hipStream_t>(stream), pos, N, n_samples, start,
                       idx, static_cast<float*>(workspace));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

size_t fc_radius_workspace_bytes(int32_t N) {
    if (N < 1) return 0;
    return radius_bytes(N);
}

int fc_radius_count(const float* pos, int32_t N, float epsilon, int32_t max_num_neighbors, void* workspace, size_t workspace_bytes,
                    void* stream) {
    if (!pos || !workspace || N < 1 || !finite_positive(epsilon) || max_num_neighbors < 1) return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < radius_bytes(N)) return FC_ERR_WORKSPACE;
    fc::Carver ws(workspace);
    const RadiusWs L = radius_ws(ws, N);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float r2 = epsilon * epsilon;
    const int K = max_num_neighbors;
    hipLaunchKernelGGL(fc::radius_count_kernel, dim3(N / fc::kRadiusThreads + 1), dim3(fc::kRadiusThreads), 0, s, pos, N, r2, K,
                       L.count, L.overfull);
    hipLaunchKernelGGL(fc::radius_select_kernel, dim3((N + 3) / 4), dim3(256), 0, s, pos, N, r2, K, L.overfull,
                       L.thresh, L.quota);
    size_t scan_bytes = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(L.scan, scan_bytes, L.count, L.offsets, N + 1, s) != hipSuccess) return FC_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

const int64_t* fc_radius_edge_count_ptr(const void* workspace, int32_t N) {
    if (!workspace || N < 1) return nullptr;
    fc::Carver ws(workspace);
    return radius_ws(ws, N).offsets + N;
}

int fc_radius_fill(const float* pos, int32_t N, float epsilon, int32_t max_num_neighbors, int64_t E, int64_t* supp_edges,
                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !workspace || N < 1 || !finite_positive(epsilon) || max_num_neighbors < 1 || E < 0) return FC_ERR_BAD_ARGUMENT;
    if (E > 0 && !supp_edges) return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < radius_bytes(N)) return FC_ERR_WORKSPACE;
    fc::Carver ws(workspace);
    const RadiusWs L = radius_ws(ws, N);
    if (E == 0) return FC_OK;
    hipLaunchKernelGGL(fc::radius_fill_kernel, dim3((N + fc::kRadiusThreads - 1) / fc::kRadiusThreads), dim3(fc::kRadiusThreads), 0,
                       static_cast<hipStream_t>(stream), pos, N, epsilon * epsilon, E, L.offsets, L.overfull, L.thresh, L.quota, supp_edges);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

size_t fc_fps_batched_workspace_bytes(int32_t N) { return fc_fps_workspace_bytes(N); }

int fc_fps_batched(const float* pos, const int64_t* pos_ptr, int32_t N, int32_t B, const int64_t* n_samples, const int64_t* start,
                   const int64_t* out_ptr, int64_t S_total, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !pos_ptr || !n_samples || !start || !out_ptr || !idx || !workspace || N < 1 || B < 1 || S_total < 1 || S_total > N)
        return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < fc_fps_batched_workspace_bytes(N)) return FC_ERR_WORKSPACE;
    hipLaunchKernelGGL(fc::fps_batched_kernel, dim3((unsigned)B), dim3(fc::kFpsThreads), 0, static_cast<hipStream_t>(stream), pos, pos_ptr,
                       N, n_samples, start, out_ptr, S_total, idx, static_cast<float*>(workspace));
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_radius_count_batched(const float* pos, const int64_t* ptr, int32_t N, int32_t B, float epsilon, int32_t max_num_neighbors,
                            void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !ptr || !workspace || N < 1 || B < 1 || !finite_positive(epsilon) || max_num_neighbors < 1 ||
        (int64_t)N + (int64_t)fc::kRadiusThreads * B >= 2147483647LL)
        return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < radius_bytes(N)) return FC_ERR_WORKSPACE;
    fc::Carver ws(workspace);
    const RadiusWs L = radius_ws(ws, N);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const float r2 = epsilon * epsilon;
    const int K = max_num_neighbors;
    // a query that no (mesh, tile) pair covers (a malformed ptr) counts nothing
    if (hipMemsetAsync(L.count, 0, (size_t)N * 8, s) != hipSuccess || hipMemsetAsync(L.overfull, 0, (size_t)N * 4, s) != hipSuccess)
        return FC_ERR_LAUNCH;
    hipLaunchKernelGGL(fc::radius_count_batched_kernel, dim3((unsigned)(N / fc::kRadiusThreads + B)), dim3(fc::kRadiusThreads), 0, s, pos,
                       ptr, B, N, r2, K, L.count, L.overfull);
    hipLaunchKernelGGL(fc::radius_select_batched_kernel, dim3((N + 3) / 4), dim3(256), 0, s, pos, ptr, B, N, r2, K, L.overfull,
                       L.thresh, L.quota);
    size_t scan_bytes = L.scan_bytes;
    if (hipcub::DeviceScan::ExclusiveSum(L.scan, scan_bytes, L.count, L.offsets, N + 1, s) != hipSuccess) return FC_ERR_LAUNCH;
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_radius_fill_batched(const float* pos, const int64_t* ptr, int32_t N, int32_t B, float epsilon, int32_t max_num_neighbors, int64_t E,
                           int64_t* supp_edges, void* workspace, size_t workspace_bytes, void* stream) {
    if (!pos || !ptr || !workspace || N < 1 || B < 1 || !finite_positive(epsilon) || max_num_neighbors < 1 || E < 0 ||
        (int64_t)N + (int64_t)fc::kRadiusThreads * B >= 2147483647LL)
        return FC_ERR_BAD_ARGUMENT;
    if (E > 0 && !supp_edges) return FC_ERR_BAD_ARGUMENT;
    if (workspace_bytes < radius_bytes(N)) return FC_ERR_WORKSPACE;
    fc::Carver ws(workspace);
    const RadiusWs L = radius_ws(ws, N);
    if (E == 0) return FC_OK;
    hipLaunchKernelGGL(fc::radius_fill_batched_kernel, dim3((unsigned)(N / fc::kRadiusThreads + B)), dim3(fc::kRadiusThreads), 0,
                       static_cast<hipStream_t>(stream), pos, ptr, B, N, epsilon * epsilon, E, L.offsets, L.overfull, L.thresh, L.quota, supp_edges);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // extern "C"
