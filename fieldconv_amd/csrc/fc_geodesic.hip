// Shortest paths over a mesh's edge graph (the edge-graph metric, not the heat method of the reference's fcutils):
//   fc_mesh_edge_lengths         len[e] = sqrt((dx*dx + dy*dy) + dz*dz) for every CSR slot, each operation rounded on its own
//                                and a correctly rounded square root, so that numpy float32 evaluates the same numbers;
//   fc_geodesic_rows             S single-source problems on one mesh -> (S,V) distances;
//   fc_geodesic_nearest          one multi-source problem per mesh of a mini-batch -> (V) distances and nearest-source labels;
//   fc_face_areas, fc_segment_sum_f32      triangle areas and sums over consecutive ranges in a fixed order (the lumped vertex
//                                mass and its sum onto the nearest sample: no float atomics, the same bits on every run).
// One solver kernel serves both launch shapes, one workgroup per problem, sweeping every vertex of the range until a sweep
// changes nothing: the least fixpoint whatever the schedule (header of fc_geodesic_relax.hpp, which also holds the ranges and
// the launch).  Labels are propagated afterwards over the fixed set of tight edges fl32(d[u] + len) == d[v]: a second
// min-propagation with the same structure.  No atomics, nothing crosses a workgroup.
#include <limits.h>
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"
#include "fc_kernels.hpp"
#include "fc_geodesic_relax.hpp"

namespace fc {

struct geo_args {
    gf_graph g;
    const int64_t* pos_ptr;      // null: every problem spans [0,V); else problem p spans [pos_ptr[p], pos_ptr[p+1])
    const int64_t* sources;      // vertex numbers
    const int64_t* src_ptr;      // null: problem p has sources[p * sources_each .. (p+1) * sources_each); else
    int64_t sources_each;        //       sources[src_ptr[p] .. src_ptr[p+1])
    int64_t n_sources;
    float* dist;                 // row of problem p: dist + p * dist_stride
    int64_t dist_stride;
    int64_t* label;              // null: distances only
    int32_t* label_ws;           // (V) labels of the ranges that do not fit LDS
    int32_t* sweeps;             // null, or (problems,2): distance sweeps, label sweeps
    int32_t lds_vertices;        // ranges of at most this many vertices belong to the LDS instantiation, larger ones to the other
};

template <bool kLds>
__global__ __launch_bounds__(kGfThreads) void geodesic_kernel(const geo_args a) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int p = blockIdx.x, t = threadIdx.x;
    // whatever the tables hold, a problem reads and writes inside [0,V) and [0,n_sources) only
    int v0, n;
    gf_mesh_range(a.pos_ptr, p, a.g.V, v0, n);
    if ((n <= a.lds_vertices) != kLds) return;          // (uniform over the workgroup) the other instantiation's problem
    int64_t s0 = gf_clamp(p * a.sources_each, 0, a.n_sources), s1 = gf_clamp(s0 + a.sources_each, s0, a.n_sources);
    if (a.src_ptr) {
        s0 = gf_clamp(a.src_ptr[p], 0, a.n_sources);
        s1 = gf_clamp(a.src_ptr[p + 1], s0, a.n_sources);
    }
    const bool want_label = a.label != nullptr;
    float* const row = a.dist + (int64_t)p * a.dist_stride + v0;
    float* const d = kLds ? reinterpret_cast<float*>(smem) : row;
    int32_t* const lab = kLds ? reinterpret_cast<int32_t*>(smem) + a.lds_vertices : a.label_ws + v0;
    const float inf = __int_as_float(0x7f800000);

    for (int i = t; i < n; i += kGfThreads) {
        d[i] = inf;
        if (want_label) lab[i] = INT_MAX;
    }
    // every thread walks the source list and takes the sources it owns: positions ascend, so the first hit is the lowest
    for (int64_t q = s0; q < s1; ++q) {
        const int64_t s = a.sources[q] - v0;
        if (s >= 0 && s < n && (int)(s % kGfThreads) == t) {
            d[s] = 0.f;
            if (want_label && lab[s] == INT_MAX) lab[s] = (int32_t)q;
        }
    }
    __syncthreads();

    int sw = 0, lsw = 0;
    for (;;) {
        int changed = 0;
        for (int i = t; i < n; i += kGfThreads) {
            int e0, e1;
            gf_row(a.g, v0 + i, e0, e1);
            const float old = d[i];
            float best = old;
            for (int e = e0; e < e1; ++e) {
                const int u = a.g.nbr[e] - v0;
                if ((unsigned)u < (unsigned)n) {
                    const float c = d[u] + a.g.len[e];
                    best = c < best ? c : best;
                }
            }
            if (best < old) {
                d[i] = best;
                changed = 1;
            }
        }
        ++sw;
        if (!__syncthreads_or(changed) || sw > n) break;
    }
    if (want_label) {
        for (;;) {
            int changed = 0;
            for (int i = t; i < n; i += kGfThreads) {
                const float dv = d[i];
                if (!(dv < inf)) continue;          // unreachable: inf + len == inf is no tight edge
                int e0, e1;
                gf_row(a.g, v0 + i, e0, e1);
                const int32_t old = lab[i];
                int32_t best = old;
                for (int e = e0; e < e1; ++e) {
                    const int u = a.g.nbr[e] - v0;
                    if ((unsigned)u < (unsigned)n && d[u] + a.g.len[e] == dv) {
                        const int32_t l = lab[u];
                        best = l < best ? l : best;
                    }
                }
                if (best < old) {
                    lab[i] = best;
                    changed = 1;
                }
            }
            ++lsw;
            if (!__syncthreads_or(changed) || lsw > n) break;
        }
    }
    for (int i = t; i < n; i += kGfThreads) {
        if (kLds) row[i] = d[i];
        if (want_label) {
            const int32_t l = lab[i];
            a.label[v0 + i] = l == INT_MAX ? -1 : (int64_t)l;
        }
    }
    if (t == 0 && a.sweeps) {
        a.sweeps[2 * (int64_t)p] = sw;
        a.sweeps[2 * (int64_t)p + 1] = lsw;
    }
}

__global__ void edge_length_kernel(const float* __restrict__ pos, const int32_t* __restrict__ src, const int32_t* __restrict__ nbr,
                                   int V, int E, float* __restrict__ len) {
#pragma clang fp contract(off)          // (plain operators: __fmul_rn / __fadd_rn are header functions that hipcc contracts)
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int u = src[e], v = nbr[e];
    if ((unsigned)u >= (unsigned)V || (unsigned)v >= (unsigned)V) {
        len[e] = __int_as_float(0x7fc00000);          // NaN: never relaxes anything
        return;
    }
    const float dx = pos[3 * (size_t)v] - pos[3 * (size_t)u], dy = pos[3 * (size_t)v + 1] - pos[3 * (size_t)u + 1],
                dz = pos[3 * (size_t)v + 2] - pos[3 * (size_t)u + 2];
    // sqrtf, not __fsqrt_rn: hipcc expands sqrtf to the correctly rounded sequence, the "intrinsic" to the bare 1-ulp v_sqrt_f32
    len[e] = sqrtf((dx * dx + dy * dy) + dz * dz);
}

// area[f] = 0.5 * |(b - a) x (c - a)|, every operation rounded on its own
__global__ void face_area_kernel(const float* __restrict__ pos, const int64_t* __restrict__ face, int V, int F, float* __restrict__ area) {
#pragma clang fp contract(off)
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    const int64_t ia = face[f], ib = face[(size_t)F + f], ic = face[2 * (size_t)F + f];
    if (ia < 0 || ia >= V || ib < 0 || ib >= V || ic < 0 || ic >= V) {
        area[f] = __int_as_float(0x7fc00000);
        return;
    }
    const float ax = pos[3 * ia], ay = pos[3 * ia + 1], az = pos[3 * ia + 2];
    const float ux = pos[3 * ib] - ax, uy = pos[3 * ib + 1] - ay, uz = pos[3 * ib + 2] - az;
    const float wx = pos[3 * ic] - ax, wy = pos[3 * ic + 1] - ay, wz = pos[3 * ic + 2] - az;
    const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
    area[f] = 0.5f * sqrtf((cx * cx + cy * cy) + cz * cz);
}

// out[k] = (((x[ptr[k]] + x[ptr[k]+1]) + ...) in float32, left to right) / divisor: one thread per range
__global__ void segment_sum_kernel(const float* __restrict__ x, const int64_t* __restrict__ ptr, int64_t N, int K, float divisor,
                                   float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= K) return;
    const int64_t b = gf_clamp(ptr[k], 0, N), e = gf_clamp(ptr[k + 1], b, N);
    float s = 0.f;
    for (int64_t i = b; i < e; ++i) s += x[i];
    out[k] = s / divisor;          // (IEEE division: hipcc's default for float32)
}

}  // namespace fc

namespace {

int geo_launch(const fc::geo_args& a, int problems, int max_range, bool labels, hipStream_t s) {
    static bool lds_ok[fc::kMaxDevices] = {};
    const size_t per_vertex = labels ? 8 : 4;
    return fc::gf_launch_pair(fc::geodesic_kernel<true>, fc::geodesic_kernel<false>, a, (unsigned)problems, max_range, a.pos_ptr != nullptr,
                              [=](size_t n) { return per_vertex * n; }, 8 * (size_t)fc::kGfLdsVertices, 0, lds_ok, s);
}

}  // namespace

extern "C" {

int32_t fc_geodesic_lds_vertices(void) { return fc::kGfLdsVertices; }

int fc_mesh_edge_lengths(const float* pos, const int32_t* src, const int32_t* nbr, int32_t V, int32_t E, float* length, void* stream) {
    if (V < 1 || E < 0 || !pos) return FC_ERR_BAD_ARGUMENT;
    if (E == 0) return FC_OK;
    if (!src || !nbr || !length) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::edge_length_kernel, dim3((unsigned)((E + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, src,
                       nbr, V, E, length);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_face_areas(const float* pos, const int64_t* face, int32_t V, int32_t F, float* area, void* stream) {
    if (V < 1 || F < 0 || !pos) return FC_ERR_BAD_ARGUMENT;
    if (F == 0) return FC_OK;
    if (!face || !area) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::face_area_kernel, dim3((unsigned)((F + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, face, V,
                       F, area);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_segment_sum_f32(const float* x, const int64_t* ptr, int64_t N, int32_t K, float divisor, float* out, void* stream) {
    if (N < 0 || K < 0 || (N > 0 && !x)) return FC_ERR_BAD_ARGUMENT;
    if (K == 0) return FC_OK;
    if (!ptr || !out) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::segment_sum_kernel, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, ptr, N, K,
                       divisor, out);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_geodesic_rows(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* sources, int32_t S,
                     float* dist, int32_t* sweeps, void* stream) {
    if (!fc::gf_graph_ok(rowptr, nbr, length, V, E) || S < 0 || (S > 0 && (!sources || !dist))) return FC_ERR_BAD_ARGUMENT;
    if (S == 0) return FC_OK;
    fc::geo_args a = {};
    a.g = {rowptr, nbr, length, V, E};
    a.sources = sources, a.sources_each = 1, a.n_sources = S;
    a.dist = dist, a.dist_stride = V;
    a.sweeps = sweeps;
    return geo_launch(a, S, V, false, static_cast<hipStream_t>(stream));
}

size_t fc_geodesic_workspace_bytes(int32_t V, int32_t max_range) {
    return V > 0 && max_range > fc::kGfLdsVertices ? sizeof(int32_t) * (size_t)V : 0;
}

int fc_geodesic_nearest(const int32_t* rowptr, const int32_t* nbr, const float* length, int32_t V, int32_t E, const int64_t* pos_ptr,
                        const int64_t* sources, const int64_t* src_ptr, int32_t S, int32_t B, int32_t max_range, float* dist,
                        int64_t* label, int32_t* sweeps, void* workspace, size_t workspace_bytes, void* stream) {
    if (!fc::gf_graph_ok(rowptr, nbr, length, V, E) || !fc::gf_batch_ok(pos_ptr, src_ptr, B, max_range, V, S, 0, S) || !sources || !dist || !label)
        return FC_ERR_BAD_ARGUMENT;
    if (!fc::gf_workspace_ok(fc_geodesic_workspace_bytes(V, max_range), workspace, workspace_bytes)) return FC_ERR_WORKSPACE;
    fc::geo_args a = {};
    a.g = {rowptr, nbr, length, V, E};
    a.pos_ptr = pos_ptr, a.sources = sources, a.src_ptr = src_ptr, a.sources_each = S, a.n_sources = S;          // (no tables: one problem, every source)
    a.dist = dist, a.dist_stride = 0;
    a.label = label, a.label_ws = static_cast<int32_t*>(workspace), a.sweeps = sweeps;
    return geo_launch(a, B, max_range, true, static_cast<hipStream_t>(stream));
}

}  // extern "C"
