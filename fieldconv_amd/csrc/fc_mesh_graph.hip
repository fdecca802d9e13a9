// The mesh's edge graph enriched by unfolded diagonals (fieldconv_amd.geodesic.mesh_edge_graph(..., diagonals=True)):
//   fc_mesh_diagonals            over the 3F half-edges sorted by (undirected side, face): the first half-edge of a run of
//                                exactly two unfolds the two faces into the plane about their shared side and, where the
//                                straight segment between the two opposite vertices crosses that side, emits the pair with the
//                                segment's length; every other slot gets the sentinel;
//   fc_mesh_graph_merge          over the directed entries (sides and diagonals, both directions) sorted by key: the first entry
//                                of a run of equal keys takes the run's smallest length.
// Sorting and compaction stay with the caller.  One thread per slot, every slot written exactly once by its own thread: no
// atomics, the same bits on every run.  Every float32 operation is rounded on its own (contraction off, IEEE division, the
// correctly rounded sqrtf), in the order the header states, so that numpy float32 evaluates the same numbers
// (tests/_diagonal_graph_ref.py).
#include "../../include/fieldconv_hip.h"
#include "fc_common.hpp"

namespace fc {

// half-edge h = 3 f + k of face (3,F): from corner k to corner k + 1, opposite corner k + 2.  false when h or a vertex is out of
// range or the face names a vertex twice.
__device__ __forceinline__ bool mg_half_edge(const int64_t* __restrict__ face, int V, int F, int64_t h, int& a, int& b, int& o) {
    if (h < 0 || h >= 3 * (int64_t)F) return false;
    const int f = (int)(h / 3), k = (int)(h % 3);
    const int64_t va = face[(size_t)k * F + f], vb = face[(size_t)((k + 1) % 3) * F + f], vo = face[(size_t)((k + 2) % 3) * F + f];
    if (va < 0 || va >= V || vb < 0 || vb >= V || vo < 0 || vo >= V || va == vb || vb == vo || vo == va) return false;
    a = (int)va, b = (int)vb, o = (int)vo;
    return true;
}

// (x, y) of vertex w in the plane of its face: x along the side from u (e / L), y >= 0 the distance from the side's line
__device__ __forceinline__ void mg_unfold(const float* __restrict__ pos, int u, int w, float ex, float ey, float ez, float L, float& x, float& y) {
#pragma clang fp contract(off)
    const float rx = pos[3 * (size_t)w] - pos[3 * (size_t)u], ry = pos[3 * (size_t)w + 1] - pos[3 * (size_t)u + 1],
                rz = pos[3 * (size_t)w + 2] - pos[3 * (size_t)u + 2];
    x = ((rx * ex + ry * ey) + rz * ez) / L;
    const float h2 = ((rx * rx + ry * ry) + rz * rz) - x * x;
    y = sqrtf(h2 > 0.f ? h2 : 0.f);
}

__global__ void diagonal_kernel(const float* __restrict__ pos, const int64_t* __restrict__ face, int V, int F, const int64_t* __restrict__ key,
                                const int64_t* __restrict__ half, int N, int32_t* __restrict__ lo, int32_t* __restrict__ hi,
                                float* __restrict__ len) {
#pragma clang fp contract(off)
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // (N may come within a block of 2^31)
    if (slot >= N) return;
    const int i = (int)slot;
    int32_t out_lo = -1, out_hi = -1;
    float out_len = __int_as_float(0x7fc00000);
    const int64_t k = key[i];
    // the first of a run of exactly two: at most two entries ahead are read
    const bool first = i == 0 || key[i - 1] != k;
    const bool two = first && i + 1 < N && key[i + 1] == k && (i + 2 >= N || key[i + 2] != k);
    int a0, b0, c, a1, b1, d;
    if (two && mg_half_edge(face, V, F, half[i], a0, b0, c) && mg_half_edge(face, V, F, half[i + 1], a1, b1, d)) {
        const int u = min(a0, b0), v = max(a0, b0);
        if (u == min(a1, b1) && v == max(a1, b1) && c != d) {          // (both half-edges lie on the side {u, v}; a face listed twice: c == d)
            const float ex = pos[3 * (size_t)v] - pos[3 * (size_t)u], ey = pos[3 * (size_t)v + 1] - pos[3 * (size_t)u + 1],
                        ez = pos[3 * (size_t)v + 2] - pos[3 * (size_t)u + 2];
            const float L2 = (ex * ex + ey * ey) + ez * ez;
            if (!(L2 == 0.f)) {
                const float L = sqrtf(L2);
                float xc, yc, xd, yd;
                mg_unfold(pos, u, c, ex, ey, ez, L, xc, yc);
                mg_unfold(pos, u, d, ex, ey, ez, L, xd, yd);
                const float s = yc + yd;
                if (!(s <= 0.f)) {
                    const float t = xc + (xd - xc) * (yc / s);
                    if (0.f < t && t < L) {
                        out_lo = min(c, d), out_hi = max(c, d);
                        out_len = sqrtf((xc - xd) * (xc - xd) + s * s);
                    }
                }
            }
        }
    }
    lo[i] = out_lo, hi[i] = out_hi, len[i] = out_len;
}

__global__ void merge_kernel(const int64_t* __restrict__ key, const float* __restrict__ length, int N, int V, uint8_t* __restrict__ head,
                             int32_t* __restrict__ src, int32_t* __restrict__ nbr, float* __restrict__ out) {
    const int64_t slot = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;          // (N may come within a block of 2^31)
    if (slot >= N) return;
    const int i = (int)slot;
    const int64_t k = key[i];
    uint8_t is_head = 0;
    int32_t s = -1, n = -1;
    float best = __int_as_float(0x7fc00000);
    if (k >= 0 && k < (int64_t)V * V && (i == 0 || key[i - 1] != k)) {
        is_head = 1, s = (int32_t)(k / V), n = (int32_t)(k % V);
        best = length[i];
        for (int j = i + 1; j < N && key[j] == k; ++j) {
            const float c = length[j];
            best = c < best ? c : best;
        }
    }
    head[i] = is_head, src[i] = s, nbr[i] = n, out[i] = best;
}

}  // namespace fc

extern "C" {

int fc_mesh_diagonals(const float* pos, const int64_t* face, int32_t V, int32_t F, const int64_t* key, const int64_t* half, int32_t N,
                      int32_t* lo, int32_t* hi, float* length, void* stream) {
    if (V < 1 || F < 0 || N < 0 || (int64_t)N > 3 * (int64_t)F || !pos) return FC_ERR_BAD_ARGUMENT;
    if (N == 0) return FC_OK;
    if (!face || !key || !half || !lo || !hi || !length) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::diagonal_kernel, dim3((unsigned)(((int64_t)N + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), pos, face,
                       V, F, key, half, N, lo, hi, length);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

int fc_mesh_graph_merge(const int64_t* key, const float* length, int32_t N, int32_t V, uint8_t* head, int32_t* src, int32_t* nbr,
                        float* out_length, void* stream) {
    if (V < 1 || N < 0) return FC_ERR_BAD_ARGUMENT;
    if (N == 0) return FC_OK;
    if (!key || !length || !head || !src || !nbr || !out_length) return FC_ERR_BAD_ARGUMENT;
    hipLaunchKernelGGL(fc::merge_kernel, dim3((unsigned)(((int64_t)N + 255) / 256)), dim3(256), 0, static_cast<hipStream_t>(stream), key, length,
                       N, V, head, src, nbr, out_length);
    return hipGetLastError() == hipSuccess ? FC_OK : FC_ERR_LAUNCH;
}

}  // extern "C"
