// The chunk-slot scheme of the per-mesh reductions (fc_segment.hip: pooling; fc_norm.hip: TangentNorm), described at the head of
// fc_segment.hip: range tables clamped where they are read, a mesh's chunk slots in closed form, the mesh of a slot or of a row by
// bisection, and the fixed combination (a_0 + a_1) + (a_2 + a_3) of the four wavefronts' running sums.
#pragma once
#include "fc_common.hpp"

namespace fc {

constexpr int kSegRows = 64;           // rows per chunk
constexpr int kSegWaves = 4;           // wavefronts per workgroup: row (partial) / chunk (finish) phases
constexpr int kSegThreads = 64 * kSegWaves;

template <typename T> struct alignas(2 * sizeof(T)) SegCx { T x, y; };

__device__ __forceinline__ int seg_bound(const int64_t* __restrict__ ptr, int b, int N) {
    const int64_t v = ptr[b];
    return (int)(v < 0 ? 0 : (v > N ? N : v));
}

// rows [p0, p1) of mesh b
__device__ __forceinline__ void seg_range(const int64_t* __restrict__ ptr, int b, int N, int& p0, int& p1) {
    p0 = seg_bound(ptr, b, N);
    p1 = max(seg_bound(ptr, b + 1, N), p0);
}

// the mesh of chunk slot g: the largest b with base(b) = ptr[b] / 64 + b <= g
__device__ __forceinline__ int seg_mesh_of_slot(const int64_t* __restrict__ ptr, int B, int N, int g) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_bound(ptr, mid, N) / kSegRows + mid <= g) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the mesh of row r: the largest b with ptr[b] <= r
__device__ __forceinline__ int seg_mesh_of_row(const int64_t* __restrict__ ptr, int B, int N, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg_bound(ptr, mid, N) <= r) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// the rows [r0, r1) of chunk slot g, a chunk of mesh b = [p0, p1); false for a spare slot (past the mesh's last chunk)
__device__ __forceinline__ bool seg_chunk_rows(int g, int b, int p0, int p1, int& r0, int& r1) {
    const long long first = (long long)p0 + (long long)(g - (p0 / kSegRows + b)) * kSegRows;
    if (first < p0 || first >= p1) return false;
    r0 = (int)first;
    r1 = (int)min(first + (long long)kSegRows, (long long)p1);
    return true;
}

// (a_0 + a_1) + (a_2 + a_3) over the four wavefronts' values of this lane; the result is valid in wavefront 0
template <typename T> __device__ __forceinline__ T seg_combine(T (*acc)[64], T s, int wave, int lane) {
    acc[wave][lane] = s;
    __syncthreads();
    return (acc[0][lane] + acc[1][lane]) + (acc[2][lane] + acc[3][lane]);
}

// the channel tiles are the grid's y extent; N + 64 B stays within 32 bits so that no slot or row index overflows
inline bool seg_shape_ok(int32_t N, int32_t B, int32_t C) {
    return N >= 0 && B >= 1 && C >= 1 && C <= 64 * 65535 && (int64_t)N + 64 * (int64_t)B < 2147483647LL;
}

inline int64_t seg_slots(int32_t N, int32_t B) { return (int64_t)N / kSegRows + B; }

}  // namespace fc
